/*
 * stnerf.h -- C ABI of libstnerf_hip.so: the MI355X (gfx950) implementation of the st-nerf layered
 * ray-march hot path.
 *
 * The reference (DarlingHang/st-nerf) has no FFI: its boundary for this path is the Python call
 * surface of LayeredRFRender.forward / layered_batchify_ray and the ops they compose.  Each entry
 * point below replaces one of those ops (cited as reference file:line, relative to
 * /root/reference) and is what a ctypes / cffi / pybind binding in the reference would bind
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - Plain C: pointers + sizes.  Every `const float*` / `float*` / `uint8_t*` / `int32_t*` argument
 *     is a DEVICE pointer unless its comment says "host".  All tensors are dense row-major fp32.
 *   - The caller owns every buffer (inputs, outputs, packed weights).  The library allocates nothing
 *     on the device and never frees caller memory.
 *   - All work is enqueued on the caller's stream (`stream` = a hipStream_t, may be NULL for the
 *     default stream).  No entry point synchronises the device or the stream.
 *   - Return value: 0 on success, a negative STNERF_E* code otherwise; stnerf_last_error() gives
 *     the message (thread-local).  Nothing throws or aborts across the ABI (the reference calls
 *     exit(-1) on a bad ray layout, modeling/layered_rfrender.py:161-163; here that is -EINVAL).
 *   - Layouts used by the chunk pipeline ("ray-major"): t[n][l][S], xyz[n][l][S][3],
 *     raw[n][l][S][4] = {r, g, b, sigma} (network outputs before any activation), mask[n][l].
 */
#ifndef STNERF_H
#define STNERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STNERF_OK 0
#define STNERF_EINVAL (-1)   /* bad argument / shape */
#define STNERF_ELAUNCH (-2)  /* HIP launch or runtime error */
#define STNERF_EARCH (-3)    /* device is not gfx950 */

#define STNERF_MAX_LAYERS 16

typedef void* stnerf_stream_t; /* hipStream_t */

/* library / device ----------------------------------------------------------------------- */
const char* stnerf_version(void);
const char* stnerf_last_error(void);
/* cu_count, lds_bytes_per_cu, clock_khz may be NULL; arch receives e.g. "gfx950" (host buffer). */
int stnerf_device_info(int* cu_count, int* lds_bytes_per_cu, int* clock_khz, char* arch, int arch_len);

/* Launch profiler: between _begin and _end every kernel launch of the entry points below is bracketed by a
 * HIP event pair recorded on the launch stream.  _end synchronises those events only and returns one record per
 * launch, in launch order (n_records = number of launches, even if larger than max_records).
 * kernel: 0 spacenet, 1 motionnet, 2 composite, 3 resample, 4 sample_coarse, 5 mlp_stage, 6 copy_layer_raw, 7 occupancy_cull,
 * 8 occupancy_build, 9 occupancy_rows, 10 ray_stop, 11 visibility_rows, 12 background_rows (kind: 1 with t_stop | 2 the per-ray flavour), 13 copy_layer_raw_listed,
 * 20 proposal_density (tag: the layer);
 * kind: the net kind for 0/1, to_dense for 6 and 13, dilate for 8, for 5 the bits deep_rgb | 2 bf16x3 |
 * 4 the row-list flavour (stnerf_mlp_stage_rows with at least one listed layer);
 * n_rays x ns = the launch's upper bound on rows (masked launches process ray_count x ns of them);
 * tag: the layer a stnerf_render_rays launch belongs to (-1 otherwise); bytes_per_ray: algorithmic HBM bytes
 * per ray for the HBM-bound kernels (2..4), 0 for the networks. */
typedef struct stnerf_profile_record {
    int32_t kernel, kind, ns, tag;
    int64_t n_rays, bytes_per_ray;
    float ms;
    int32_t pad_;
} stnerf_profile_record;
int stnerf_profile_begin(void);
int stnerf_profile_end(stnerf_profile_record* records_host, int max_records, int* n_records);

/* Per-layer edit applied to sample points (inverse of the box edit), host struct passed by value
 * inside stnerf_scene.  modeling/layered_rfrender.py:293-303 (coarse) and :467-475 (fine). */
typedef struct stnerf_layer_edit {
    float shift[3];  /* x -= shift              (only if has_shift) */
    float scale;     /* x = (x - pivot) / scale + pivot   (only if has_scale) */
    int32_t has_shift;
    int32_t has_scale;
} stnerf_layer_edit;

/* Per-layer rigid rotation R about `centre`, applied to the layer's content after its scale and shift: the box, the radiance
 * field and the field's view dependence turn together.  Not in the reference (render/layered_neural_renderer.py:19-24 stores
 * `rotation` and never reads it).  Rendering it means the layer sees the ray in its own frame, and is then rendered unrotated:
 *     m = R^T (row-major), c = centre, q = o - c
 *     o'[r] = ((m[3r] q[0] + m[3r+1] q[1]) + m[3r+2] q[2]) + c[r]
 *     d'[r] =  (m[3r] d[0] + m[3r+1] d[1]) + m[3r+2] d[2]                    r = 0, 1, 2
 * every product, sum and difference a separate IEEE fp32 operation in this order (no fused multiply-add).  For the layer,
 * (o', d') take the place of (o, d) in the slab test, in the sample points t d' + o' of both passes (ahead of the point
 * un-edit) and in the direction the colour branch encodes (stnerf_rgb_ray_bias).  Depths are the ray's own (the map is
 * rigid), so the depth merge and the compositor see nothing new; the RNG keys, the mask bits and the frame ids stay as
 * they are.  m must be a rotation: the caller checks (stnerf_amd.LayeredRFRender.layer_ray_transforms does).
 * Host struct; the entries that take one read `enabled` first: 0 = this layer is not rotated. */
typedef struct stnerf_layer_rotation {
    float m[9];       /* R^T, row-major */
    float centre[3];
    int32_t enabled;
} stnerf_layer_rotation;

/* Which rays of a view a call works on.  Local ray i of a call is GLOBAL ray
 *     first + i                                    (stripe == 0: one contiguous window)
 *     first + (i / stripe) * period + i % stripe   (stripe  > 0: stripes of `stripe` rays, one every `period` rays --
 *                                                   what rank r of G takes of a view split into interleaved stripes:
 *                                                   first = r * stripe, period = G * stripe)
 * The global index selects the pixel (stnerf_generate_rays) and keys the device RNG (stnerf_sample_coarse,
 * stnerf_resample, stnerf_render_rays), so an image does not depend on how its rays are cut into launches, chunks
 * or GPU shards.  The three numbers travel as (first_ray | ray_index_base, ray_index_stripe, ray_index_period). */

/* a1 + a2: pinhole rays of the n rays of the window (first_ray, stripe, period) of an h x w view, row-major over
 * (row, col), written as [origin(3), dir(3), frame_ids(n_frame_cols)] with `ray_stride` floats per
 * ray.  Replaces utils/render_helpers.py:42-128 (generate_rays), utils/ray_sampling.py:22-72 and
 * data/datasets/ray_dataset.py:276-281.  Kinv = inverse intrinsics (host, 9 floats, row-major),
 * T = camera-to-world (host, 16 floats), frame_ids host array of n_frame_cols floats (or NULL). */
int stnerf_generate_rays(const float* Kinv_host, const float* T_host, int h, int w, int64_t first_ray,
                         int64_t ray_index_stripe, int64_t ray_index_period, int64_t n,
                         const float* frame_ids_host, int n_frame_cols, float* rays, int ray_stride,
                         stnerf_stream_t stream);

/* a5: ray / 8-corner-box slab test.  layers/RaySamplePoint.py:8-62 (intersection).
 * boxes: [l][8][3] shared by all rays (box_ray_stride = 0) or per ray (box_ray_stride = l*24).
 * far_near out: [n][l][2] = (far, near), (-1000,-1000) on a miss. */
int stnerf_intersect(const float* rays, int64_t n, int ray_stride, const float* boxes,
                     int64_t box_ray_stride, int l, float* far_near, stnerf_stream_t stream);

/* a5 + a6 (+ the point un-edit of a4): stratified jittered coarse samples of every layer.
 * layers/RaySamplePoint.py:70-107 (RaySamplePoint.forward).
 * jitter: [l][n][n1] uniform draws to REPLAY (the reference's torch.rand tensors), or NULL to draw
 * on the device: Philox4x32-10 keyed by (seed, global ray index, layer, sample) -- independent
 * of chunking (global index: see the ray-window note above).  edits: host array of l entries or NULL; pivot: host, 3 floats.
 * Outputs: t[n][l][n1], xyz[n][l][n1][3] (may be NULL), mask[n][l]: bit 0 = the reference's ray_mask (|bin width| > 1e-5,
 * :105); bit 1 = a HINT for stnerf_composite: the ray misses the layer's box altogether (both slab hits -1000, :53-62), so
 * every depth of the (ray, layer) pair is exactly -1000 and the compositor need not read them to find that out (40 % of a
 * nine-layer ray's depth bytes).  Consumers of the mask as the reference's boolean take `mask & 1`; stnerf_compact_rays and
 * stnerf_composite do.  A mask without hints (bit 1 clear everywhere) is always valid; a caller-made mask must be strictly 0 / 1
 * (any other value is read as hit-bit + hint).  stnerf_render_rays clears the hints before it returns: its `mask` output is 0 / 1. */
int stnerf_sample_coarse(const float* rays, int64_t n, int ray_stride, const float* boxes,
                         int64_t box_ray_stride, int l, int n1, const float* jitter, uint64_t seed,
                         int64_t ray_index_base, int64_t ray_index_stripe, int64_t ray_index_period,
                         const stnerf_layer_edit* edits_host, const float* pivot_host, float* t, float* xyz,
                         uint8_t* mask, stnerf_stream_t stream);
/* The same with per-layer rotations (stnerf_layer_rotation above): rotations_host = host array of l entries, or NULL = none,
 * which is what stnerf_sample_coarse forwards.  A call without an enabled entry launches the kernels of the plain call. */
int stnerf_sample_coarse_rot(const float* rays, int64_t n, int ray_stride, const float* boxes,
                             int64_t box_ray_stride, int l, int n1, const float* jitter, uint64_t seed,
                             int64_t ray_index_base, int64_t ray_index_stripe, int64_t ray_index_period,
                             const stnerf_layer_edit* edits_host, const float* pivot_host,
                             const stnerf_layer_rotation* rotations_host, float* t, float* xyz,
                             uint8_t* mask, stnerf_stream_t stream);

/* Ragged work: list of rays whose mask[ray][layer] is set.  Replaces the boolean-mask indexing
 * (and its host sync) at modeling/layered_rfrender.py:344-353,400-413,497-510,555-563.
 * ray_list[layer][n] (int32; row `layer` gets the hits, in no particular order), ray_count[layer].
 * ray_count must be zeroed by the caller before the call (it is accumulated with atomics). */
int stnerf_compact_rays(const uint8_t* mask, int64_t n, int l, int32_t* ray_list, int32_t* ray_count,
                        stnerf_stream_t stream);

/* Network weights ------------------------------------------------------------------------- */
#define STNERF_NET_SPACE 0      /* SpaceNet(use_time=False)  modeling/spacenet.py:16-86  */
#define STNERF_NET_SPACE_TIME 1 /* SpaceNet(use_time=True)                               */
#define STNERF_NET_MOTION 2     /* MotionNet(c_input=4)  modeling/motion_net.py:7-32     */
#define STNERF_NET_SPACE_DEEP 3      /* SpaceNet(use_time=False, deep_rgb=True)  modeling/spacenet.py:68-79 */
#define STNERF_NET_SPACE_TIME_DEEP 4 /* SpaceNet(use_time=True,  deep_rgb=True)                             */
#define STNERF_NET_IS_SPACE(kind) ((kind) == STNERF_NET_SPACE || (kind) == STNERF_NET_SPACE_TIME || \
                                   (kind) == STNERF_NET_SPACE_DEEP || (kind) == STNERF_NET_SPACE_TIME_DEEP)
#define STNERF_NET_USES_TIME(kind) ((kind) == STNERF_NET_SPACE_TIME || (kind) == STNERF_NET_SPACE_TIME_DEEP)
#define STNERF_NET_IS_DEEP(kind) ((kind) == STNERF_NET_SPACE_DEEP || (kind) == STNERF_NET_SPACE_TIME_DEEP)

/* Bytes of the packed (kernel-layout) weight blob of one network. */
int64_t stnerf_packed_bytes(int kind);
/* stnerf_pack_net with every tensor and the destination IN DEVICE MEMORY (weights_dev / biases_dev: host arrays of device pointers;
 * same tensors, same blob, bit for bit): one memset + one kernel on `stream`, no host round trip -- what a training loop calls after
 * every optimizer.step() (round 5). */
int stnerf_pack_net_device(int kind, const float* const* weights_dev, const float* const* biases_dev, int n_tensors, void* dst_dev,
                           int64_t dst_bytes, stnerf_stream_t stream);
/* The A operands of the fused backward chains (stnerf_train_spacenet_dx / stnerf_train_motionnet_dx): `count` (<= 12) sections of one
 * destination blob, each an nn.Linear weight W (n_out x n_in, row stride ldw floats, device memory) as [n_out / 4][n_pad][4] --
 * dst[dst_off + ((o / 4) n_pad + n) 4 + o % 4] = W[o][n], zero for n_in <= n < n_pad -- or, n_pad == 0, a plain copy of its n_out x n_in
 * floats (the heads).  One launch, no host round trip: a training loop rebuilds them after every optimizer.step(). */
typedef struct stnerf_transpose_section {
    const float* w;
    int64_t ldw;
    int64_t dst_off;   /* floats */
    int32_t n_out, n_in, n_pad;
} stnerf_transpose_section;
int stnerf_pack_transposed(const stnerf_transpose_section* sections, int count, float* dst_dev, int64_t dst_floats, stnerf_stream_t stream);
/* Repack reference-layout tensors (nn.Linear: weight (out,in) row-major, bias (out)) into the
 * kernel layout.  HOST -> HOST; the caller uploads `dst` to the device (any allocator).
 * SpaceNet order (10 tensors): stage1.{0,2,4,6}, stage2.{0,2,4}, density_net.0, rgb_net.{1,3};
 * deep_rgb kinds (12 tensors): ..., density_net.0, rgb_net.{1,3,5,7}.
 * MotionNet order (6): motion_net.{0,2,4,6,8,10}.  Checkpoint key names: SURVEY.md section 5. */
int stnerf_pack_net(int kind, const float* const* weights_host, const float* const* biases_host,
                    int n_tensors, void* dst_host, int64_t dst_bytes);

/* a7 + a9: fused positional encoding + SpaceNet MLP (exact f32 MFMA).  modeling/spacenet.py:101-160.
 * Exact-f32 blobs (stnerf_pack_net): the stnerf_mlp_stage kernel on a single layer (bit-identical to that layer of a stage launch
 * without STNERF_STAGE_SIGMOID_RGB), no queue word needed.
 * Work list: ray slot s in [0, count) -> ray j = ray_list ? ray_list[s] : s, where count =
 * ray_count ? min(*ray_count, n_rays) : n_rays; every ray contributes ns samples.
 *   pos   of (j,k): xyz  + j*xyz_ray_stride  + 3k      (3 floats)
 *   dir   of  j   : dirs + j*dirs_ray_stride           (3 floats)
 *   time  of  j   : times + j*times_ray_stride         (1 float; kinds with time only)
 *   out   of (j,k): raw  + j*raw_ray_stride  + 4k      = {r, g, b, sigma}, no activation
 * All strides in floats. */
int stnerf_spacenet_fwd(int kind, const void* packed, int64_t n_rays, int ns, const int32_t* ray_list,
                        const int32_t* ray_count, const float* xyz, int64_t xyz_ray_stride,
                        const float* dirs, int64_t dirs_ray_stride, const float* times,
                        int64_t times_ray_stride, float* raw, int64_t raw_ray_stride, float* ray_bias,
                        stnerf_stream_t stream);
/* The same for a rotated layer: rotation_host = ONE struct (stnerf_layer_rotation, of the net's layer) or NULL; the colour branch then
 * encodes d' = R^T d (only `m` is read: a direction has no centre).  xyz are the caller's points, as always. */
int stnerf_spacenet_fwd_rot(int kind, const void* packed, int64_t n_rays, int ns, const int32_t* ray_list,
                            const int32_t* ray_count, const float* xyz, int64_t xyz_ray_stride,
                            const float* dirs, int64_t dirs_ray_stride, const float* times,
                            int64_t times_ray_stride, float* raw, int64_t raw_ray_stride, float* ray_bias,
                            const stnerf_layer_rotation* rotation_host, stnerf_stream_t stream);

/* The per-ray part of rgb_net.1 (modeling/spacenet.py:80-86,141-151): the layer reads the 256 backbone features of a
 * sample and the encodings of the ray's direction and frame id -- the same 27 (+ 21) numbers for every sample of the ray
 * (:115,118 repeat them).  out[j][0..127] = bias + W[:, 256:] * relu([PE_4(dir_j), PE_10(time_j)]) for the listed rays j
 * (rows of other rays are left untouched); the exact-f32 MLP kernels add row j behind the layer's product
 * (the split-bf16 ones likewise).  stnerf_spacenet_fwd and stnerf_mlp_stage call this themselves into their `ray_bias` workspaces
 * ([n_rays][128] floats per layer, 16-byte aligned); exported for tests and for callers that want the table. */
int stnerf_rgb_ray_bias(int kind, const void* packed, int64_t n_rays, const int32_t* ray_list, const int32_t* ray_count,
                        const float* dirs, int64_t dirs_ray_stride, const float* times, int64_t times_ray_stride,
                        float* out, stnerf_stream_t stream);
/* The same with the direction turned first: rotation_host = ONE stnerf_layer_rotation or NULL (none: the plain call's kernel). */
int stnerf_rgb_ray_bias_rot(int kind, const void* packed, int64_t n_rays, const int32_t* ray_list, const int32_t* ray_count,
                            const float* dirs, int64_t dirs_ray_stride, const float* times, int64_t times_ray_stride,
                            float* out, const stnerf_layer_rotation* rotation_host, stnerf_stream_t stream);

/* a7 + a8: fused positional encoding (with the fractional-time lerp) + MotionNet MLP (exact f32 MFMA: the MotionNet of
 * stnerf_mlp_stage and of stnerf_train_motionnet_fwd, one persistent launch).
 * modeling/motion_net.py:34-71.  Same work list as above.  flow (may be NULL) gets the 3-vector at
 * flow + j*flow_ray_stride + 3k.  `add_to_xyz` is a set of STNERF_MOTION_* bits: ADD_TO_XYZ updates the
 * point in place (xyz += flow), which is what modeling/layered_rfrender.py:355-356,509-510 do; PLAIN_TIME
 * selects MotionNet(input_time=False) (motion_net.py:61-62: PE of [xyz, t] as given, no floor/ceil lerp),
 * the flavour of bkgd_time_deform_net (layered_rfrender.py:92-93). */
#define STNERF_MOTION_ADD_TO_XYZ 1
#define STNERF_MOTION_PLAIN_TIME 2
int stnerf_motionnet_fwd(const void* packed, int64_t n_rays, int ns, const int32_t* ray_list,
                         const int32_t* ray_count, float* xyz, int64_t xyz_ray_stride,
                         const float* times, int64_t times_ray_stride, float* flow,
                         int64_t flow_ray_stride, int add_to_xyz, stnerf_stream_t stream);

/* "bf16x3": the packed form of a network for the split-bf16 arithmetic of stnerf_mlp_stage (STNERF_STAGE_BF16X3;
 * csrc/mlp_bf16x3.hip; packers: csrc/pack_bf16x3.hip).  modeling/spacenet.py:45-86, modeling/motion_net.py:20-32 are plain fp32 nn.Linear layers: every
 * weight (host side, here) and every activation (in the kernel) is split into three bf16 numbers, x = x0 + x1 + x2 --
 * 8 + 8 + 8 significand bits, i.e. exact for every finite fp32 value inside bf16's exponent range (|x| <= 3.39e38: above
 * bf16's largest finite value the leading piece rounds to inf; residual pieces below 2^-133 flush, an error < 2^-16 of
 * the smallest normal number), with fp32's exponent range: no |W| limit, no activation limit, no overflow flag -- and a
 * product is evaluated with its six leading cross terms on the bf16 MFMA (dropped terms <= 2^-24 |a b|),
 * fp32 accumulate.  Same tensors as stnerf_pack_net; the blob = [the exact-f32 blob of stnerf_pack_net | bias vectors and
 * head weights in the kernel's LDS order | the MFMA layers' weights as bf16 triples in consumption order].  All net
 * kinds.  The device copy must be 1 KB aligned.
 * Edge semantics (tests/test_gpu_stage.py::test_stage_kernels_edge_semantics, tests/test_bf16x3_pack_cpu.py):
 *   weights / biases: STNERF_EINVAL for NaN, +-inf and |w| > 3.3895e38 (bf16's largest finite value; fp32's top 0.4 % cannot be split);
 *   fp32-subnormal weights are accepted, pieces below 2^-133 flush (absolute error < 2^-133 per weight);
 *   sample points must be FINITE (the sampler's and the resampler's are).  Neither stage kernel propagates NaN / inf the way ATen does:
 *   their ReLU is an integer max on the bit pattern (one instruction; -inf and sign-bit NaNs become 0), and the bf16 split turns what is
 *   left into zero pieces.  A sample with a NaN / inf coordinate therefore gets, in bf16x3, the FINITE outputs of a network whose first
 *   layer's activations are zero (the biases' response: the same values for every such sample) where ATen returns NaN; the exact-f32
 *   kernel (the stage kernel, also behind stnerf_spacenet_fwd) returns NaN for a +inf coordinate and finite values for -inf and NaN.  Likewise activations that overflow fp32 (|x| > 3.4e38: ATen carries +-inf / NaN on) give unspecified
 *   values for that sample.  In every case ONLY that sample is affected: every other sample of the launch, of the same wave included,
 *   is bit-identical to a launch without it.  Subnormal activations and products behave as in the exact-f32 kernel up to the flush. */
int64_t stnerf_packed_bytes_bf16x3(int kind);
int stnerf_pack_net_bf16x3(int kind, const float* const* weights_host, const float* const* biases_host,
                           int n_tensors, void* dst_host, int64_t dst_bytes);
/* The same blob, bit for bit, from tensors IN DEVICE MEMORY into a 1 KB-aligned device destination (host arrays of device pointers;
 * one memset + two kernels on `stream`): what a training loop calls after every optimizer.step() when its forward runs in split
 * bf16 (stnerf_train_spacenet_fwd_bf16x3; round 6).  No finiteness check (no host round trip): a weight stnerf_pack_net_bf16x3 would
 * refuse gives NaN pieces and NaN outputs. */
int stnerf_pack_net_bf16x3_device(int kind, const float* const* weights_dev, const float* const* biases_dev, int n_tensors,
                                  void* dst_dev, int64_t dst_bytes, stnerf_stream_t stream);

/* a8 + a9 for a whole network stage of the pipeline (coarse or fine, modeling/layered_rfrender.py:340-418 / :495-576):
 * ONE persistent launch evaluates every listed layer -- one workgroup per CU pops work items (128 rows of a layer; the
 * MotionNet of a deformed layer runs in front of its SpaceNet on the same rows, the flow stays on chip) from a device-side
 * queue (csrc/stage_entry.hip).  A wave owns 32 samples and the activations never leave its registers.  Two arithmetics:
 * exact f32 (csrc/mlp_wave.hip, the default; results bit-identical to stnerf_motionnet_fwd(ADD_TO_XYZ) followed by
 * stnerf_spacenet_fwd per layer, except that the deformed points are NOT written back to xyz) and, with
 * STNERF_STAGE_BF16X3, split-bf16 (csrc/mlp_bf16x3.hip: every fp32 operand as three bf16 pieces, six bf16 MFMAs per
 * product, two fp32 accumulators -- fp32's exponent range, no range limits, closer to an fp64 evaluation than an fp32
 * fma chain is; every net must then be a blob of stnerf_pack_net_bf16x3, 1 KB aligned).  `queue`: one zeroed uint32 on
 * the device.  `ray_bias`: workspace of n_layers x n_rays x 128 floats (16-byte aligned) for the per-ray part of
 * rgb_net.1 (stnerf_rgb_ray_bias).
 * flags: STNERF_STAGE_DEEP_RGB = the SpaceNets are of a *_DEEP kind; STNERF_STAGE_SIGMOID_RGB = store sigmoid(rgb)
 * instead of the raw colour head output (torch.sigmoid of layers/render_layer.py:47 moved into the network epilogue,
 * where it is free; pair it with stnerf_composite_params.rgb_activated = 1); STNERF_STAGE_BF16X3 as above. */
#define STNERF_STAGE_DEEP_RGB 1
#define STNERF_STAGE_SIGMOID_RGB 2
#define STNERF_STAGE_BF16X3 4
typedef struct stnerf_stage_layer {
    const void* space;         /* packed SpaceNet (kind given by use_time and the deep_rgb argument)                 */
    const void* motion;        /* packed MotionNet evaluated first on the same rows (xyz + flow), or NULL            */
    const int32_t* ray_list;   /* compacted hit rays of the layer (stnerf_compact_rays) or NULL = every ray          */
    const int32_t* ray_count;
    const float* xyz;          /* [n][ns][3] with ray stride xyz_ray_stride                                         */
    float* raw;                /* [n][ns][4] with ray stride raw_ray_stride                                         */
    const float* times;        /* frame id of ray j at times[j * times_ray_stride]; NULL if neither net takes it    */
    int32_t use_time;          /* the SpaceNet is of a *_TIME kind                                                  */
    int32_t motion_flags;      /* STNERF_MOTION_PLAIN_TIME                                                          */
    const stnerf_layer_rotation* rotation;  /* host; NULL (a zeroed struct) or !enabled: none.  The layer's ray-bias launch
                                             * encodes R^T dir (stnerf_rgb_ray_bias_rot); the stage kernel is the same   */
} stnerf_stage_layer;
int stnerf_mlp_stage(const stnerf_stage_layer* layers_host, int n_layers, int64_t n_rays, int ns, const float* dirs,
                     int64_t dirs_ray_stride, int64_t times_ray_stride, int64_t xyz_ray_stride,
                     int64_t raw_ray_stride, int flags, uint32_t* queue, float* ray_bias, stnerf_stream_t stream);
/* The same stage with a ROW LIST on some of its layers (the sample cull, below: stnerf_occupancy_rows writes the lists).
 * rows_host: n_layers entries beside layers_host, or NULL.  Entry i with row_list != NULL: queue slot i has *row_count rows (never
 * more than n_rays x ns are walked), and row r of it is sample k = v & 255 of ray v >> 8, v = row_list[r] -- instead of
 * (ray_list[r / ns], r % ns).  Points, outputs, frame ids and the ray-bias row are addressed by (ray, k) as ever, so a listed row
 * gets the 16 bytes the unlisted launch writes for that sample, and nothing is written for a sample that is on no list.  The
 * layer's ray_list / ray_count still name the rays its ray-bias rows are made for: every ray of the row list must be on it.
 * Listed and unlisted layers share one launch.  A list needs ns <= 256 and n_rays <= 2^23 (STNERF_EINVAL).  NULL, or no entry with
 * a list, is stnerf_mlp_stage: the same kernels.  With a list the row-list flavours run (csrc/mlp_wave_rows.hip,
 * csrc/mlp_bf16x3_rows.hip: the same kernel text under another name, with this locate step). */
typedef struct stnerf_stage_rows {
    const int32_t* row_list;   /* device; NULL: the layer's rows are ray_count x ns */
    const int32_t* row_count;  /* device */
} stnerf_stage_rows;
int stnerf_mlp_stage_rows(const stnerf_stage_layer* layers_host, const stnerf_stage_rows* rows_host, int n_layers, int64_t n_rays, int ns,
                          const float* dirs, int64_t dirs_ray_stride, int64_t times_ray_stride, int64_t xyz_ray_stride,
                          int64_t raw_ray_stride, int flags, uint32_t* queue, float* ray_bias, stnerf_stream_t stream);

/* a7 standalone: NeRF positional encoding [x, sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(2^(L-1) x)],
 * each block `dim` wide.  utils/dimension_kernel.py:3-73 (Trigonometric_kernel.__call__).  In the render
 * path the encoding is fused into the MLP kernels; this entry point serves the op-level API.
 * x[n][dim] -> y[n][dim*(include_input + 2*n_freq)].  Same < 1 ulp sin/cos as the fused kernels. */
int stnerf_encode(const float* x, int64_t n, int dim, int n_freq, int include_input, float* y,
                  stnerf_stream_t stream);

/* a12 standalone: gen_weight(sigma, delta), layers/render_layer.py:8-17.  sigma[n][S] raw, delta[n][S]
 * -> weights[n][S] = alpha * exclusive cumprod(1 - alpha + 1e-10), alpha = 1 - exp(-relu(sigma) delta). */
int stnerf_gen_weight(const float* sigma, const float* delta, int64_t n, int S, float* weights,
                      stnerf_stream_t stream);

/* a10 + a11 + a12: post-network density edits, per-layer composite, cross-layer merge by depth
 * and merged composite, one pass per ray.  layers/render_layer.py:8-58 (gen_weight,
 * VolumeRenderer.forward); modeling/layered_rfrender.py:414-448 (coarse), :538-606 (fine). */
typedef struct stnerf_composite_params {
    float border;                              /* last interval, BOARDER_WEIGHT            */
    float near;                                /* model.near                               */
    int32_t fine;                              /* 0: coarse-stage rules, 1: fine-stage     */
    int32_t cut_negative_t;                    /* coarse: performer sigma[t<0]=0  (:414)   */
    float threshold[STNERF_MAX_LAYERS];        /* sigma < threshold -> 0 (retiming)        */
    int32_t use_threshold[STNERF_MAX_LAYERS];
    float sigma_scale[STNERF_MAX_LAYERS];      /* fine: layer 2 *= alpha (:575-576), else 1 */
    int32_t rgb_activated;                     /* 1: raw[..][0..2] already hold sigmoid(rgb) (stnerf_mlp_stage with
                                                * STNERF_STAGE_SIGMOID_RGB applies it in the network epilogue);
                                                * 0: raw network output, torch.sigmoid is applied here (render_layer.py:47) */
    int32_t evaluated[STNERF_MAX_LAYERS];      /* 0: layer's nets were skipped (hidden): raw is not read;
                                                * 1: evaluated on the rays `mask` marks (performers, :397-413);
                                                * 2: evaluated on EVERY ray, `mask` is not consulted (the background:
                                                *    bkgd_spacenet runs on all rays, :382-392, and is composited even
                                                *    where ray_mask[0] is False -- a ray through an edge of its box) */
} stnerf_composite_params;

/* t[n][l][S], raw[n][l][S][4], mask[n][l] (NULL = all set; a clear bit means "not evaluated":
 * rgb = sigma = 0 as the reference's zero tensors, :398-399).
 * Outputs (any may be NULL): layer_out[n][l][5] = {color(3), depth, acc}; mixed_out[n][5];
 * weights[n][l][S] per-layer weights (needed by stnerf_resample); order[n][l*S] int32 = source
 * index (layer*S + k) of each merged sample (torch.sort's index, ties broken by source index).
 * scratch: n bytes of device memory or NULL (contents on return unspecified).  With scratch the rays with a single live
 * layer (about half of a view) are composited first by a latency-pipelined kernel that needs no LDS, the others by the
 * register / insertion-merge kernel -- in two launches when a merged list of all l layers would not fit the LDS at full
 * occupancy (e.g. 9 x 192 samples); without scratch that kernel takes every ray in one launch.  The `order` output and
 * layers of more than 192 samples take the LDS-staged kernel.  Same images and weights bit for bit on every route. */
int stnerf_composite(const float* t, const float* raw, const uint8_t* mask, int64_t n, int l, int S,
                     const stnerf_composite_params* params_host, float* layer_out, float* mixed_out,
                     float* weights, int32_t* order, uint8_t* scratch, stnerf_stream_t stream);

/* stnerf_composite with the in-scene layer passes (stnerf_composite forwards here with two NULLs and launches what it always did).
 * The merged composite gives every sample of the stably sorted union the weight w = alpha T (after the density edits, the fine
 * stage's `t < near` cut on the merged copy, and with the deltas of the MERGED list, `border` last).
 *   merged_weights[n][l][S]: that weight, stored at the sample's SOURCE index (layer-major, as `weights`); exact zeros for a layer
 *     that takes no part on the ray (no network output and every depth -1000).  Needs mixed_out.
 *   scene_out[n][l][5] = sum_k merged_weights {r, g, b, t, 1} per layer, in layer_out's layout: layer i's premultiplied colour,
 *     weighted depth and alpha INSIDE the mixed image, occluded by and occluding the others (layer_out[i] is layer i alone).  r, g,
 *     b are the colours the compositor used (sigmoid(rgb), or raw's own with rgb_activated); a layer without network output on the
 *     ray (hidden, missed, a grazing hit) gets five exact zeros.  sum_i scene_out[i] equals mixed_out up to the order of the fp32
 *     sums.  Needs merged_weights (STNERF_EINVAL before any launch otherwise); one more HBM-bound launch, 24 B per sample.
 * Either may be NULL.  Same bits on every route, and the other outputs are the bits of stnerf_composite. */
int stnerf_composite_scene(const float* t, const float* raw, const uint8_t* mask, int64_t n, int l, int S,
                           const stnerf_composite_params* params_host, float* layer_out, float* mixed_out,
                           float* weights, int32_t* order, uint8_t* scratch, float* merged_weights, float* scene_out,
                           stnerf_stream_t stream);

/* backward of stnerf_composite -- what loss.backward() (engine/layered_trainer.py:277) does to
 * VolumeRenderer.forward / gen_weight (layers/render_layer.py:8-58) and to the merge gather
 * (modeling/layered_rfrender.py:425-429, :587-592) through ATen: given g_layer[n][l][5] and g_mixed[n][5] = dLoss /
 * d{colour(3), depth, acc} of every layer's composite and of the merged one (either may be NULL), writes
 * d_raw[n][l][S][4] = dLoss / d{rgb(3), sigma} of the raw network outputs (zeros where a layer was not evaluated on a ray).
 * t, raw, mask, params: exactly what the forward call got; order[n][l*S]: the forward's `order` output (required with
 * g_mixed).  The density edits act as in the reference's in-place writes: an overwritten sigma gets no gradient, layer 2's
 * `*= alpha` scales it.  Depths get none (the sampler and sample_pdf are detached, :314-315, :460-461).
 * torch.cumprod's backward is reproduced as ATen computes it without zeros in the input (reversed cumsum / input; the
 * 1e-10 of gen_weight keeps every factor positive).  csrc/render_bwd.hip. */
int stnerf_composite_bwd(const float* t, const float* raw, const uint8_t* mask, const int32_t* order, int64_t n, int l, int S,
                         const stnerf_composite_params* params_host, const float* g_layer, const float* g_mixed,
                         float* d_raw, stnerf_stream_t stream);

/* The launch plan stnerf_composite follows for a shape (host arithmetic only, no GPU needed): plan[0] 1 = the LDS-staged
 * kernel alone; [1] single-layer pre-pass (0 none, 1 / 2 = its two instantiations); [2] launches of the merge kernel (1 or
 * 2); [3] layers the first launch's merged list holds; [4] 1 = scratch is cleared first; [5], [6] waves per workgroup and
 * dynamic LDS bytes of the first launch (or of the staged kernel); [7], [8] of the second launch (0 without one).
 * STNERF_EINVAL when a ray of l * S samples does not fit the LDS (the message says how much it needs). */
int stnerf_composite_plan(int l, int S, int with_scratch, int with_order, int64_t* plan);

/* a13 (+ the sort/merge and point generation of layered_rfrender.py:459-475): inverse-CDF
 * resampling of every layer.  utils/sample_pdf.py:18-63.
 * t[n][l][n1] coarse depths, weights[n][l][n1] coarse per-layer weights (interior [1:-1] used),
 * u: [l][n][n2] uniform draws to replay, or NULL -> device Philox (seed, global ray index, stream 1).
 * Outputs: t_fine[n][l][n1+n2] ascending; xyz_fine[n][l][n1+n2][3] (may be NULL) = un-edited points;
 * optional debug/parity outputs z_new[n][l][n2] (unsorted new samples), inds[n][l][n2] int32
 * (searchsorted index), cdf[n][l][n1-1].
 * Exactness: pdf = (w + 1e-5) / torch.sum(w + 1e-5) with the sum in ATen's CPU reduction order (8-float vectors x 4
 * interleaved accumulators), cdf = torch.cumsum accumulated in fp64 and rounded per prefix as ATen's CPU kernel does:
 * cdf, inds and z_new are bit-equal to the reference's CPU evaluation of utils/sample_pdf.py on the same (t, w, u).
 * mask (may be NULL): stnerf_sample_coarse's byte per (ray, layer).  A pair whose "missed" hint (bit 1) is set is SKIPPED:
 * every one of its depths is -1000, so are its resampled depths, and nobody reads them -- stnerf_composite with the same mask
 * never looks at a flagged layer's depths, the networks list hit rays only: its t_fine / xyz_fine rows are left unwritten
 * (16 B x S per pair: at nine layers most of this kernel's bytes were such constant fills).  Without hints (NULL, or bit 1 clear)
 * a pair whose depths are all -1000 gets t_fine = -1000 and the matching points, as before. */
int stnerf_resample(const float* t, const float* weights, int64_t n, int l, int n1, int n2,
                    const float* u, uint64_t seed, int64_t ray_index_base, int64_t ray_index_stripe,
                    int64_t ray_index_period, const float* rays,
                    int ray_stride, const stnerf_layer_edit* edits_host, const float* pivot_host, const uint8_t* mask,
                    float* t_fine, float* xyz_fine, float* z_new, int32_t* inds, float* cdf,
                    stnerf_stream_t stream);
/* The same with per-layer rotations (host array of l stnerf_layer_rotation, or NULL = none, which is what stnerf_resample
 * forwards): the points of a rotated layer are t d' + o', then un-edited.  Depths do not change.  A call with an enabled
 * entry runs the kernel flavour that carries the box edits; one without launches what the plain call launches. */
int stnerf_resample_rot(const float* t, const float* weights, int64_t n, int l, int n1, int n2,
                        const float* u, uint64_t seed, int64_t ray_index_base, int64_t ray_index_stripe,
                        int64_t ray_index_period, const float* rays,
                        int ray_stride, const stnerf_layer_edit* edits_host, const float* pivot_host,
                        const stnerf_layer_rotation* rotations_host, const uint8_t* mask,
                        float* t_fine, float* xyz_fine, float* z_new, int32_t* inds, float* cdf,
                        stnerf_stream_t stream);

/* ---- backward pass of the two networks (csrc/train.hip) ------------------------------------------------------
 * What engine/layered_trainer.py:192-217's loss.backward() does to modeling/spacenet.py:45-86 / modeling/motion_net.py:20-32
 * through ATen (addmm_backward: two mm + a sum per nn.Linear), as f32 MFMA GEMMs (v_mfma_f32_32x32x2_f32, exact fp32
 * products and accumulation) on matrices the caller owns.  stnerf_amd.modeling.autograd strings them into
 * torch.autograd.Functions for SpaceNet / MotionNet: the forward is recomputed chunk by chunk with every layer's input kept
 * (sample-major [rows][ld]), then walked backwards.  All row strides (ld*) in floats; operand rows that are read with 16-byte
 * vectors need ld % 4 == 0, a 16-byte aligned base and allocations covering whole vectors (pad columns: weights zero).
 *
 * y[m][n] = act(sum_k x[m][k] w[n][k] + bias[n])   (w: the reference's nn.Linear layout, out x in; relu = 0 / 1) */
int stnerf_train_linear_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, int64_t m, int n, int k,
                            int relu, float* y, int64_t ldy, stnerf_stream_t stream);
/* dx[m][k] (+)= (sum_n dy[m][n] w[n][k]) * (mask[m][k] > 0): `mask` = the stored post-ReLU tensor that fed this layer (the
 * ReLU backward of the PRODUCING layer folded in; NULL: none); accumulate = 1 adds to dx (a tensor with two consumers). */
int stnerf_train_linear_dx(const float* dy, int64_t lddy, const float* w, int64_t ldw, int64_t m, int n, int k, const float* mask,
                           int64_t ldmask, int accumulate, float* dx, int64_t lddx, stnerf_stream_t stream);
/* dw[n][k] (+)= sum_m dy[m][n] x[m][k];  db[n] (+)= sum_m dy[m][n] (db may be NULL).  The samples are cut into <= 256 slices
 * of >= 256 samples (as many as give the launch two workgroups per CU), reduced by separate workgroups into `workspace`, then
 * summed in slice order: deterministic, no atomics. */
int64_t stnerf_train_dw_workspace_bytes(int64_t m, int n, int k);
int stnerf_train_linear_dw(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t m, int n, int k, float* dw, int64_t lddw,
                           float* db, int accumulate, void* workspace, int64_t workspace_bytes, stnerf_stream_t stream);
/* Every weight and bias gradient of a network in ONE launch (+ one for the reduction): `count` (<= 16) layers whose dy / x have
 * the same m rows -- what loss.backward() accumulates into the .grad of every nn.Linear of modeling/spacenet.py:45-86 or
 * modeling/motion_net.py:20-32 --, same operand rules and the same result contract as stnerf_train_linear_dw (dw[n][k] (+)= dy^T
 * x, db[n] (+)= column sums of dy, db may be NULL).  csrc/train_dw.hip: a WAVE keeps a 128 x 128 tile of one dw in its
 * accumulator registers (row blocks of 128 -- one block of 32 for a layer of <= 4 outputs --, column pieces of 128, the last piece
 * 96 / 64 / 32 wide) and streams a range of samples past it, operands straight from the row-major matrices (no LDS); sample ranges
 * are sized by a tile's MFMA count so that the launch's <= 1024 waves finish together (>= 64 samples each); partial tiles are summed
 * in range order: deterministic, no atomics.  At most 64 tiles and 100 reduction segments (tiles + bias row blocks) per call.
 * Columns of dy / x beyond n / k may be read (up to the tile's width: into the row's padding, the next row, never beyond the last
 * row's round4 end); they only reach outputs that are not stored. */
typedef struct stnerf_dw_problem {
    const float* dy;   /* [m][lddy], n columns */
    int64_t lddy;
    const float* x;    /* [m][ldx], k columns */
    int64_t ldx;
    float* dw;         /* [n][lddw] */
    int64_t lddw;
    float* db;         /* [n] or NULL */
    int32_t n, k;
} stnerf_dw_problem;
int64_t stnerf_train_dw_batch_workspace_bytes(const stnerf_dw_problem* problems, int32_t count, int64_t m);
/* How stnerf_train_dw_batch runs these problems (host arithmetic only, the same plan): bundles_out[0] = 2 x 2 bundles in split bf16,
 * [1] = 2 x 2 bundles in f32, [2] = shared-input bundles (two 256-output layers whose 64-column tiles read the same columns of one matrix). */
int stnerf_train_dw_batch_plan(const stnerf_dw_problem* problems, int32_t count, int64_t m, int32_t* bundles_out);
int stnerf_train_dw_batch(const stnerf_dw_problem* problems, int32_t count, int64_t m, int32_t accumulate, void* workspace,
                          int64_t workspace_bytes, stnerf_stream_t stream);
/* Positional encoding (utils/dimension_kernel.py:54-73) of x[src][0..dim) into columns [col0, col0 + dim (include_input + 2
 * n_freq)) of y[rows][ldy] (a column block of a layer's input matrix: the skip connection of modeling/spacenet.py:128 and
 * rgb_net's input :141-151 are assembled in place).  rows_per_src = ns repeats a ray's encoding on its ns samples (:115,118);
 * relu = 1 applies rgb_net's leading in-place ReLU to the encoded columns (:80); lerp_col >= 0 treats that input column as
 * a frame id and blends the encodings of floor(t) and floor(t) + 1 (modeling/motion_net.py:52-60), -1: none. */
int stnerf_train_encode(const float* x, int64_t ldx, int dim, int n_freq, int include_input, int64_t rows, int rows_per_src, int relu,
                        int lerp_col, float* y, int64_t ldy, int col0, stnerf_stream_t stream);
/* dx[row][j] (+)= sum_features dy[row][col0 + feature] d enc_feature / d x_j for the first dim_out input columns. */
int stnerf_train_encode_bwd(const float* x, int64_t ldx, int dim, int n_freq, int include_input, int64_t rows, const float* dy,
                            int64_t lddy, int col0, int dim_out, int accumulate, float* dx, int64_t lddx, stnerf_stream_t stream);

/* The SpaceNet's backward as fused launches (csrc/train_wave.hip, csrc/mlp_wave.hip; networks without deep_rgb):
 *
 * stnerf_train_spacenet_fwd = stnerf_mlp_stage on ONE SpaceNet (exact f32, the arithmetic of the training forward), every ray
 * evaluated, which ALSO writes each layer's input as it passes through the registers: act[s][row][ld_act[s]], row = ray * ns + k,
 * s = 0 .. 6 the post-ReLU outputs of stage1.0 .. stage2.4 (256 columns), s = 7 of rgb_net.1 (128 columns), and pe[row][ld_pe] =
 * PE_10(pos) (63 columns + one zero) -- the right operands of the weight gradients -- and relu_bits (uint32, may be NULL): stage s's
 * plane starts at relu_bits + s * relu_bits_stride and holds 8 words per row: the ReLU masks [act_s > 0] as bits, 32 bytes per row and
 * layer in the lane order of the wave kernels (csrc/mlp_wave.hip StoreTap) -- all stnerf_train_spacenet_dx reads of the activations
 * (a row range of a larger launch's planes is addressed by offsetting the pointer and keeping the stride).  The matrices are the caller's (16-byte aligned, row
 * strides multiples of 4 floats), e.g. column blocks of wider ones (stage2.0's input [h4 | PE]).
 * act_host / ld_act_host: host arrays of 8 device pointers / strides.  queue, ray_bias: as for stnerf_mlp_stage (one layer).
 *
 * stnerf_train_spacenet_dx: from d_raw[rows][4] = dLoss / d {r, g, b, sigma} walks the layers backwards, a wave carrying the
 * gradient of its 32 rows from layer to layer in registers: d act_{s-1} = (d act_s * [act_s > 0]) W_s (threshold_backward, then
 * addmm_backward's grad_input), the masks from relu_bits.  dy[s][row][ld_dy[s]] receives the masked gradient = dLoss / d
 * (pre-activation of that layer), the left operand of its weight gradient (stnerf_train_linear_dw); dpe (may be NULL) receives
 * dLoss / d PE(pos) (64 columns), for stnerf_train_encode_bwd.  wt: the transposed weights, sections [out / 4][N][4] (N = inputs
 * padded to a multiple of 32) at offsets_host[0] (rgb_net.1's 256 backbone columns: out 128), [1 .. 7] (stage1.0: N 64; stage1.2 ..
 * 1.6: N 256; stage2.0: N 320 = [h4 | PE]; stage2.2, 2.4: N 256), then density_net.0's 256 weights at [8] and the colour head's
 * [3][128] at [9] (float offsets, multiples of 4); stnerf_amd.modeling.autograd builds it. */
int stnerf_train_spacenet_fwd(int kind, const void* packed, int64_t n_rays, int ns, const float* xyz, int64_t xyz_ray_stride,
                              const float* dirs, int64_t dirs_ray_stride, const float* times, int64_t times_ray_stride, float* raw,
                              int64_t raw_ray_stride, float* const* act_host, const int32_t* ld_act_host, float* pe, int32_t ld_pe,
                              uint32_t* relu_bits, int64_t relu_bits_stride, uint32_t* queue, float* ray_bias, stnerf_stream_t stream);
/* The same launch in split bf16 (round 6): stnerf_mlp_stage's STNERF_STAGE_BF16X3 kernel (csrc/mlp_bf16x3.hip) with the same tap --
 * raw is bit-identical to what stnerf_mlp_stage / the render pipeline give for these samples in that arithmetic, the stored
 * activations are that kernel's fp32 layer outputs (fp32-faithful: within a few ulp of the exact-f32 launch's), the masks are
 * theirs.  `packed`: a blob of stnerf_pack_net_bf16x3[_device], 1 KB aligned.  Everything else as above. */
int stnerf_train_spacenet_fwd_bf16x3(int kind, const void* packed, int64_t n_rays, int ns, const float* xyz, int64_t xyz_ray_stride,
                                     const float* dirs, int64_t dirs_ray_stride, const float* times, int64_t times_ray_stride, float* raw,
                                     int64_t raw_ray_stride, float* const* act_host, const int32_t* ld_act_host, float* pe, int32_t ld_pe,
                                     uint32_t* relu_bits, int64_t relu_bits_stride, uint32_t* queue, float* ray_bias,
                                     stnerf_stream_t stream);
int stnerf_train_spacenet_dx(const float* wt, const uint32_t* offsets_host, const float* d_raw, int64_t rows, const uint32_t* relu_bits,
                             int64_t relu_bits_stride, float* const* dy_host, const int32_t* ld_dy_host, float* dpe, int32_t ld_dpe,
                             stnerf_stream_t stream);
/* stnerf_train_spacenet_dx in split bf16 (round 6; csrc/train_bf16x3.hip: train_space_dx_bx_kernel -- the forward kernel's machinery with
 * the transposed weights as a bf16x3 stream through the LDS ring, the masks fetched per work item by LDS-DMA): same inputs, same dy
 * matrices, fp32-faithful values.  The weights come as ONE blob, stnerf_pack_dx_bf16x3_device(kind, weights_dev (the network's 10
 * weight tensors in reference layout, host array of device pointers), 10, with_dpos, dst (1 KB aligned,
 * stnerf_packed_bytes_dx_bf16x3(kind, with_dpos) bytes)).  with_dpos != 0: the chain goes on to PE(pos) and leaves
 * dLoss / d PE(pos) as the SUM of two 64-column matrices, dpe (d y0 W_stage1.0) and dpe_skip (d y4 W_stage2.0[:, 256:]) -- the caller
 * adds them (the exact-f32 kernel carries one through four layers in registers this kernel does not have); with_dpos == 0: both NULL. */
int64_t stnerf_packed_bytes_dx_bf16x3(int kind, int with_dpos);
int stnerf_pack_dx_bf16x3_device(int kind, const float* const* weights_dev, int n_tensors, int with_dpos, void* dst_dev, int64_t dst_bytes,
                                 stnerf_stream_t stream);
int stnerf_train_spacenet_dx_bf16x3(const void* packed_dx, int with_dpos, const float* d_raw, int64_t rows, const uint32_t* relu_bits,
                                    int64_t relu_bits_stride, float* const* dy_host, const int32_t* ld_dy_host, float* dpe, int32_t ld_dpe,
                                    float* dpe_skip, int32_t ld_dpe_skip, stnerf_stream_t stream);

/* The MotionNet's backward (modeling/motion_net.py:20-71 under loss.backward()) as the same two launches (csrc/train_wave.hip):
 *
 * stnerf_train_motionnet_fwd: flow[row][3] = MotionNet(xt[row] = {x, y, z, frame id}) with the arithmetic of the inference kernels'
 * MotionNet (exact f32; motion_flags: STNERF_MOTION_PLAIN_TIME or 0, as stnerf_motionnet_fwd), writing what the backward needs as
 * the rows pass through the registers: enc[row][ld_enc] = the 84 encoded features (+ 4 zeros; fractional frame ids blended as
 * motion_net.py:52-60 does), act[s][row][ld_act[s]] = the post-ReLU outputs of motion_net.0, .2, .4, .6, .8 (128 columns), and
 * relu_bits: stage s's plane at relu_bits + s * relu_bits_stride, 4 words per row (the masks [act_s > 0], 16 bytes per row and layer,
 * in the lane order of the wave kernels).
 *
 * stnerf_train_motionnet_dx: from d_flow[rows][4] (dLoss / d flow in columns 0 .. 2) back through the five hidden layers with the
 * gradient in registers: dy[s][row][ld_dy[s]] = dLoss / d (pre-activation of motion_net.{0,2,4,6,8}[s]) (128 columns), the left
 * operands of the weight gradients, and denc[row][ld_denc] (may be NULL; 96 columns written, 84 meaningful) = dLoss / d encoding
 * for stnerf_train_encode_bwd.  wt: transposed sections [128 / 4][128][4] of motion_net.0 (its 84 inputs zero-padded to 128) and
 * .2 .. .8 at offsets_host[0 .. 4], the flow head's [3][128] as it is at [5] (float offsets, multiples of 4). */
int stnerf_train_motionnet_fwd(const void* packed, const float* xt, int64_t rows, int motion_flags, float* flow, float* enc, int32_t ld_enc,
                               float* const* act_host, const int32_t* ld_act_host, uint32_t* relu_bits, int64_t relu_bits_stride,
                               stnerf_stream_t stream);
int stnerf_train_motionnet_dx(const float* wt, const uint32_t* offsets_host, const float* d_flow, int64_t rows, const uint32_t* relu_bits,
                              int64_t relu_bits_stride, float* const* dy_host, const int32_t* ld_dy_host, float* denc, int32_t ld_denc,
                              stnerf_stream_t stream);

/* The whole chunk pipeline of LayeredRFRender.forward (modeling/layered_rfrender.py:141-734) behind one call:
 * coarse sampler -> mask compaction -> [MotionNet] -> SpaceNets -> composite/merge -> resample -> [MotionNet] ->
 * fine SpaceNets -> composite/merge, all enqueued on `stream` into a caller-provided workspace.  Host-side
 * box interpolation / editing (l x 8 x 3 numbers, :190-242) stays with the caller, who passes the edited boxes
 * and the inverse point edits.  Packed-network pointers are device blobs of stnerf_pack_net[_bf16x3].
 * Entries of stnerf_nets may ALIAS: two layers may name one blob (and one MotionNet).  That is how a layer INSTANCE -- a performer
 * shown a second time with its own frame-id column, box, edit, rotation, shown flag and opacity -- is expressed at this level: the
 * library never compares or groups network pointers, every per-layer input above is indexed by the layer, and the RNG is keyed by
 * the layer index, so an instance draws its own jitter. */
typedef struct stnerf_nets {
    const void* bkgd;                           /* bkgd_spacenet            (STNERF_NET_SPACE)               */
    const void* bkgd_fine;                      /* bkgd_spacenet_fine                                        */
    const void* space[STNERF_MAX_LAYERS];       /* [i] = spacenets[i-1], i >= 1 ([0] unused)                 */
    const void* space_fine[STNERF_MAX_LAYERS];  /* [i] = spacenets_fine[i-1]                                 */
    const void* motion[STNERF_MAX_LAYERS];      /* [i] = time_deform_nets[i-1] (use_deform_time only);
                                                   [0] = bkgd_time_deform_net (bkgd_use_deform_time only)    */
} stnerf_nets;

typedef struct stnerf_render_params {
    int32_t l, n1, n2;            /* layers incl. background, coarse / fine sample counts                     */
    int32_t ray_stride;           /* floats per ray: 6 + l (retiming) or 7                                   */
    int32_t retiming;             /* 1: frame id of layer i in column 6+i; 0: per-ray frame id in column 6   */
    int32_t only_coarse;
    int32_t use_deform_time, use_space_time;
    int32_t precision;            /* 3: bf16x3 (split-bf16, stnerf_mlp_stage with STNERF_STAGE_BF16X3; nets packed by
                                     stnerf_pack_net_bf16x3) -- what the Python boundary selects by default; 0: exact f32 MFMA, one
                                     persistent stnerf_mlp_stage launch per stage; 2: exact f32, one launch per network
                                     (stnerf_motionnet_fwd / stnerf_spacenet_fwd: the same arithmetic, for A/B runs of
                                     the scheduling).  (1 was the retired split-fp16 mode: rejected.) */
    int32_t has_edits;            /* edits_* / pivot are meaningful                                          */
    int32_t bkgd_use_deform_time; /* BKGD_USE_DEFORM_TIME: nets.motion[0] warps the background samples (:358-367) */
    int32_t bkgd_use_space_time;  /* BKGD_USE_SPACE_TIME: background SpaceNets take the frame id (needs use_space_time, :382-390) */
    int32_t deep_rgb;             /* DEEP_RGB && USE_SPACE_TIME (:35): every SpaceNet blob is of a *_DEEP kind */
    int32_t shown[STNERF_MAX_LAYERS];                 /* display_layers (:99-112); [0] ignored               */
    float border, near, alpha;                        /* BOARDER_WEIGHT, model.near, model.alpha             */
    float density_threshold, bkgd_density_threshold;  /* applied in retiming mode only, as the reference     */
    uint64_t seed;                                    /* device RNG (used where jitter / u are NULL)         */
    int64_t ray_index_base, ray_index_stripe, ray_index_period;  /* ray window of rays[0..n) (see above)     */
    stnerf_layer_edit edits_coarse[STNERF_MAX_LAYERS]; /* :293-303 */
    stnerf_layer_edit edits_fine[STNERF_MAX_LAYERS];   /* :467-475 */
    float pivot[3];
} stnerf_render_params;

int64_t stnerf_render_workspace_bytes(int64_t n, int l, int n1, int n2, int only_coarse);
/* Outputs: mixed_*[n][5], layer_*[n][l][5] = {colour(3), depth, acc}; mask[n][l].  jitter [l][n][n1] / u [l][n][n2]
 * replay uniform draws (NULL = device RNG).  With only_coarse the fine outputs may be NULL. */
int stnerf_render_rays(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                       const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                       const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                       float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                       stnerf_stream_t stream);

/* One layer's slice of the ray-major network outputs raw[n][l][ns][4] <-> a dense buffer dense[n][ns][4]: to_dense != 0 copies
 * raw[:, layer] out, to_dense == 0 copies it back in (the other layers' slices are not touched).  16 bytes per sample and lane;
 * both pointers 16-byte aligned.  HBM-bound: 32 ns bytes of traffic per ray. */
int stnerf_copy_layer_raw(float* raw, int64_t n, int l, int layer, int ns, float* dense, int to_dense, stnerf_stream_t stream);

/* The background layer's network outputs of a fixed view, kept by the caller across frames.  While the rays, the background box
 * and edit, the seed, the sample counts, the arithmetic and the background networks (and, where it takes one, its frame id) stay
 * what they were, layer 0's raw outputs of both stages are the same bits in every frame whatever the performers do: their frame
 * ids, boxes, edits and shown flags, alpha and the density thresholds act on other layers or after the networks.  The CALLER
 * decides when that holds (stnerf_amd.BackgroundCache keys it on the host); the library only moves the data.
 *   raw_coarse[n][n1][4], raw_fine[n][n1+n2][4] (unused with only_coarse, may be NULL then): dense fp32, 16-byte aligned, exactly
 *   what the stage kernels stored for layer 0 (before any density edit).
 *   mode STNERF_BKGD_CACHE_OFF: as without a cache; _CAPTURE: render as usual and copy layer 0's slices out; _REUSE: leave layer 0
 *   out of both network stages and copy the slices in.  Everything else (sampler, compaction, compositor, resampler) runs for every
 *   layer in every mode, so a _REUSE frame is bit-identical to the frame rendered without a cache. */
#define STNERF_BKGD_CACHE_OFF 0
#define STNERF_BKGD_CACHE_CAPTURE 1
#define STNERF_BKGD_CACHE_REUSE 2
typedef struct stnerf_bkgd_cache {
    float* raw_coarse;
    float* raw_fine;
    int32_t mode;
} stnerf_bkgd_cache;
/* stnerf_render_rays with a background cache (NULL: none; stnerf_render_rays forwards here with NULL).  The cache arguments are
 * checked on the host before anything is launched. */
int stnerf_render_rays_cached(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                              const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                              const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                              float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                              const stnerf_bkgd_cache* cache_host, stnerf_stream_t stream);
/* stnerf_render_rays_cached with per-layer rotations (host array of params->l stnerf_layer_rotation, or NULL = none, which is
 * what the two entries above forward): the table goes to the sampler, the resampler and every ray-bias launch of both passes,
 * in all three precisions; the stage kernels, the compositor and the workspace are untouched, and a call without an enabled
 * entry makes exactly the launches it made before.  The same table serves both passes, so MotionNet reuse holds.  A background
 * cache is the CALLER's to key: layer 0's rotation is an input of the background's raw outputs, the performers' are not. */
int stnerf_render_rays_rot(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                           const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                           const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                           float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                           const stnerf_bkgd_cache* cache_host, const stnerf_layer_rotation* rotations_host,
                           stnerf_stream_t stream);
/* stnerf_render_rays_rot with the in-scene layer passes of the FINAL stage (fine, or coarse with only_coarse): scene_out[n][l][5]
 * as stnerf_composite_scene defines it, or NULL = none, which is what the entries above forward and which makes exactly the
 * launches they made before.  The merged weights live in the final stage's point buffer, which is dead once that stage's
 * networks have run: the workspace is stnerf_render_workspace_bytes, unchanged. */
int stnerf_render_rays_scene(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                             const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                             const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                             float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                             const stnerf_bkgd_cache* cache_host, const stnerf_layer_rotation* rotations_host,
                             float* scene_out, stnerf_stream_t stream);
/* stnerf_render_rays_scene with a per-layer opacity table: layer_alpha_host[params->l] floats on the host, or NULL = none, which is
 * what the entries above forward and which makes exactly the launches and results they made before.  Entry i multiplies layer i's
 * density in the FINE composite (stnerf_composite_params.sigma_scale[i]), where the reference's `alpha` acts on layer 2 alone
 * (:575-576); the coarse composite, and so an only_coarse call, ignores the table as it ignores `alpha`.  While a table is given
 * params->alpha is ignored.  Every entry must be finite and >= 0: checked on the host before anything is launched. */
int stnerf_render_rays_opacity(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                               const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                               const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                               float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                               const stnerf_bkgd_cache* cache_host, const stnerf_layer_rotation* rotations_host,
                               float* scene_out, const float* layer_alpha_host, stnerf_stream_t stream);

/* ---- occupancy grids (csrc/occupancy.hip) ---------------------------------------------------------------
 * One bit per cell of a performer's box, and a cull that drops a (ray, performer) pair when none of its coarse sample points
 * lies in an occupied cell.  Not in the reference beyond utils/vis_density.py (a density grid of a box).
 *   Grid.  res = (Rx, Ry, Rz) cells, 1..256 per axis, spanning the axis-aligned bounds lo, hi (fp32) of the 8 corners of the
 *   layer's UNEDITED box at the layer's frame id.  Cell (x, y, z) is bit c & 31 of word c >> 5, c = (z Ry + y) Rx + x; the table
 *   has ceil(Rx Ry Rz / 32) uint32 words, the unused high bits of the last word 0.
 *   Point to cell, per axis a:  c_a = min(max((int)floorf((p_a - lo_a) * inv_a), 0), R_a - 1),  inv_a = (float)R_a / (hi_a - lo_a)
 *   computed once on the host in fp32; the subtraction and the product are separate fp32 operations (no fused multiply-add).
 *   A point with a NaN coordinate counts as occupied.
 *   Build.  sigma_c / sigma_f: fp32 [Rz+1][Ry+1][Rx+1] (either may be NULL), the densities of the layer's coarse / fine SpaceNet at
 *   the grid's vertices (vertex j of axis a at lo_a + j ((hi_a - lo_a) / R_a) in fp32, vertex R_a at hi_a itself).  A vertex is
 *   dense when !(sigma <= threshold) in either array (a NaN is dense), a cell occupied when one of its 8 corners is dense; the
 *   grid is the occupied set grown by `dilate` cells in Chebyshev distance, 0 <= dilate <= 4.
 *   Cull.  For every layer with a grid (bits != NULL) and every ray whose mask[ray][layer] has bit 0 set: if none of the n1 points
 *   xyz[ray][layer][k] -- the points the networks would be given: after the ray's rotation and the scale / shift un-edit, before
 *   the MotionNet -- lies in an occupied cell, bit 0 is cleared.  Nothing else is written: bit 1, the layers without a grid, the
 *   depths and the points stay as they are.  The pair is then in the state of a ray that grazes the box (bit 0 clear, bit 1 clear,
 *   depths real): no network runs on it, its depths still take part in the merge and the resampling.
 *   Layer 0 cannot carry a grid (STNERF_EINVAL): the background runs on every ray whatever its mask.
 * Host struct; a table has l entries; bits == NULL: the layer is not culled.  Checked on the host before any launch: res in
 * range, inv_cell finite and positive, bits 4-byte aligned, no grid on layer 0. */
typedef struct stnerf_occupancy {
    const uint32_t* bits;   /* device */
    int32_t res[3];         /* Rx, Ry, Rz */
    float lo[3];
    float inv_cell[3];
} stnerf_occupancy;
int stnerf_occupancy_build(const float* sigma_c, const float* sigma_f, const int32_t res[3], float threshold, int dilate,
                           uint32_t* bits, stnerf_stream_t stream);
/* xyz[n][l][n1][3], mask[n][l]; one launch per layer with a grid, one wave per ray.  counts_or_null: device, int32 [l][2] =
 * (pairs tested, pairs culled) per layer, ACCUMULATED (one 64-bit add per wave: 8-byte aligned; the caller zeroes it). */
int stnerf_occupancy_cull(const float* xyz, int64_t n, int l, int n1, const stnerf_occupancy* table_host, uint8_t* mask,
                          int32_t* counts_or_null, stnerf_stream_t stream);
/*   Sample cull.  For a layer i >= 1 with a grid, a network stage of ns samples (the coarse stage: n1, the fine stage: n1 + n2) and
 *   every ray on the layer's compacted list (the whole-ray cull above has run): sample k is LISTED when the point xyz[ray][i][k] --
 *   the point the networks would be given: after rotation and un-edit, before the MotionNet -- lies in an occupied cell or has a
 *   NaN coordinate, by the point-to-cell rule above, unchanged.  A listed sample is evaluated exactly as without the cull.  A sample
 *   that is not listed gets raw[ray][i][k] = {0, 0, 0, 0}, four exact zero words, and no network runs on it.  Nothing else changes:
 *   depths, points, masks, the resampler, the compositor and the scene passes see a `raw` buffer and behave as they always did
 *   (sigma = 0 gives alpha = 0: a skipped sample weighs nothing, its depth still takes part in the merge).
 *
 *   Row lists (csrc/sample_rows.hip).  Four entries make the row list of ONE layer in ONE network stage of ns samples:
 *   stnerf_occupancy_rows (here), stnerf_visibility_rows, stnerf_background_rows and stnerf_background_ray_rows (below).  They differ
 *   in which tests make a sample LISTED -- its ray's flag byte, !(t > t_stop[ray]), its point's cell -- and in where their rays come
 *   from; this contract is common to all four.
 *     Arguments.  xyz / t / raw: the LAYER's slices (as in stnerf_stage_layer) of the stage's points, depths and outputs, each with
 *     its ray stride in floats; raw 16-byte aligned, its stride a multiple of 4 floats.  The tested rays are the first
 *     min(n, *ray_count) slots of ray_list (ray_count NULL: n of them; ray_list NULL: the slot is the ray), or, for the two
 *     background entries, the rays 0 .. n-1.  Per-ray arrays (t_stop, ray_flags) are indexed by the ray.
 *     row_list[capacity] int32: one word (ray << 8) | k per listed sample.  The rows of one ray are contiguous and ascending in k;
 *     the order of the rays is free (runs of 16 slots land in the order of their atomic adds: it changes from run to run).
 *     raw: the zero float4 {0, 0, 0, 0} of every sample of every tested ray that is NOT listed -- and nothing else of raw.
 *     row_count int32: zeroed by the call itself, on the stream, then the number of words.
 *     counts_or_null: device, int64, 8-byte aligned, two words += (samples tested, samples not listed), ACCUMULATED (the caller
 *     zeroes them): row `layer` of a [..][2] table for the two entries that take a layer, the array itself for the background's.
 *     Limits, STNERF_EINVAL for all four: ns outside 1..256 (the sample takes 8 bits of a word), n > 2^23 (the ray takes 23),
 *     capacity < n * ns, raw or counts misaligned, a null pointer among the required ones, a bad grid.
 *     One launch: a persistent grid of at most 2048 workgroups of 256; a wave takes runs of 16 slots, keeps their ballots in scalar
 *     registers, reserves the run's range of the list with one vector atomic add, and adds to each counter once.
 * stnerf_occupancy_rows: listed = the grid test alone; rays from the layer's work list; grid_host: the layer's entry, with bits.
 * It also refuses layer 0 (the background is never listed by this entry). */
int stnerf_occupancy_rows(const int32_t* ray_list, const int32_t* ray_count, int64_t n, int layer, const float* xyz, int64_t xyz_ray_stride,
                          int ns, const stnerf_occupancy* grid_host, float* raw, int64_t raw_ray_stride, int32_t* row_list,
                          int64_t capacity, int32_t* row_count, int64_t* counts_or_null, stnerf_stream_t stream);
/* stnerf_render_rays_opacity with an occupancy table (host array of params->l entries, or NULL = none, which is what the entries
 * above forward and which makes exactly the launches they made, in a workspace of the same size).  The cull runs after the coarse
 * sampler and before the ray compaction; both passes, the compositor, the resampler, the scene passes and the returned mask
 * follow from the mask as they always did.  The stage kernels are untouched: a culled frame is the same kernels on fewer rows. */
int stnerf_render_rays_occupancy(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                                 const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                                 const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                                 float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                                 const stnerf_bkgd_cache* cache_host, const stnerf_layer_rotation* rotations_host,
                                 float* scene_out, const float* layer_alpha_host, const stnerf_occupancy* occupancy_host,
                                 int32_t* counts_or_null, stnerf_stream_t stream);
/* stnerf_render_rays_occupancy with the sample cull.  samples_host: params->l flags (host) or NULL = none, which is what
 * stnerf_render_rays_occupancy forwards and which makes exactly the launches it made, in a workspace of
 * stnerf_render_workspace_bytes.  samples_host[i] != 0 needs a grid on layer i (STNERF_EINVAL otherwise) and sample-culls it in both
 * stages: stnerf_occupancy_rows on the coarse points after the ray cull and the compaction, and on the fine points after the
 * resampler, each right before its stage, which then walks the row list (stnerf_mlp_stage_rows).  A sample-culled layer's MotionNet
 * runs fused, inside the stage kernel and on listed rows only (it takes no part in the MotionNet reuse of the split-bf16 stages).
 * The workspace grows by one row list per sample-culled layer: stnerf_render_workspace_bytes_samples.  params->precision == 2 (one
 * launch per network) with a sample-culled layer: STNERF_EINVAL.  sample_counts_or_null: device, int64 [l][2] = (samples tested,
 * samples skipped) per layer over both stages, accumulated. */
int64_t stnerf_render_workspace_bytes_samples(int64_t n, int l, int n1, int n2, int only_coarse, const int32_t* samples_host);
int stnerf_render_rays_samples(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                               const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                               const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                               float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                               const stnerf_bkgd_cache* cache_host, const stnerf_layer_rotation* rotations_host,
                               float* scene_out, const float* layer_alpha_host, const stnerf_occupancy* occupancy_host,
                               int32_t* counts_or_null, const int32_t* samples_host, int64_t* sample_counts_or_null,
                               stnerf_stream_t stream);

/* ---- early ray termination (csrc/termination.hip, csrc/sample_rows.hip) -------------------------------
 * Opt-in, inference only, the FINE stage only: fine samples that the coarse pass shows to lie behind enough opacity get zero
 * outputs instead of a network evaluation.  Not in the reference.
 *   Stop depth.  One ray after the coarse composite: t[l][n1] its coarse depths, wM[l][n1] its coarse MERGED weights at source
 *   index (stnerf_composite_scene's merged_weights, after the coarse density edits).  The l n1 samples are merged by depth,
 *   stably, ties broken by the source index layer n1 + k -- the compositor's `order`; every layer's depths ascend, so this is an
 *   l-way merge in which the lower layer wins a tie.  The merged list is walked j = 0, 1, .. with ONE fp32 accumulator and one
 *   fp32 add per step, in this order: A <- A + wM[src(j)].  j* is the first j with !(1.0f - A > tau) -- a NaN stops the walk.
 *   t_stop is the depth of merged sample j* + 1 (sample j's weight belongs to the interval that ends at the next merged depth);
 *   t_stop = +inf when there is no such j or j* is the last sample.  tau: fp32 in [0, 1).  Depths are never NaN.
 *   Hidden sample.  Sample k of layer i of the fine stage is HIDDEN when t_f[ray][i][k] > t_stop[ray]; a NaN depth is not
 *   hidden.  A hidden sample gets raw_f[ray][i][k] = {0, 0, 0, 0}, four exact zero words; no network and no MotionNet runs on it.
 *   A sample that is not hidden is evaluated exactly as without termination.  Nothing else changes: depths, points, masks, the
 *   compositor and the scene passes see a `raw` buffer and behave as they always did.
 *   With a sample-culling grid on the layer a sample is LISTED when it is listed by the grid rule above AND not hidden.
 * stnerf_ray_stop: t[n][l][n1], merged_weights[n][l][n1] -> t_stop[n].  One launch, one lane per ray (an l-way merge in
 * registers).  STNERF_EINVAL: a null pointer, l outside 1..STNERF_MAX_LAYERS, n1 < 1, tau outside [0, 1) or NaN. */
int stnerf_ray_stop(const float* t, const float* merged_weights, int64_t n, int l, int n1, float tau, float* t_stop,
                    stnerf_stream_t stream);
/* stnerf_visibility_rows makes one layer's row list under this rule (the row-list contract above): listed = not hidden, and with
 * a grid the grid test; rays from the layer's work list; t and t_stop[n] required.
 *   grid_host_or_null: the layer's grid, or NULL (or bits == NULL) = no grid: every sample that is not hidden is listed, and xyz
 *     is not read (it may be NULL);
 *   layer 0 allowed (without a grid; ray_list NULL = rays 0 .. n-1).
 * It also refuses a grid on layer 0 and a grid without xyz. */
int stnerf_visibility_rows(const int32_t* ray_list, const int32_t* ray_count, int64_t n, int layer, const float* xyz,
                           int64_t xyz_ray_stride, const float* t, int64_t t_ray_stride, const float* t_stop, int ns,
                           const stnerf_occupancy* grid_host_or_null, float* raw, int64_t raw_ray_stride, int32_t* row_list,
                           int64_t capacity, int32_t* row_count, int64_t* counts_or_null, stnerf_stream_t stream);
/* stnerf_render_rays_samples with early ray termination.  terminate_host: params->l flags (host) or NULL = none, which is what
 * stnerf_render_rays_samples forwards and which -- like a table of zeros, or only_coarse -- makes exactly the launches it made, in
 * a workspace of stnerf_render_workspace_bytes_samples.  With a flag set: the coarse composite also writes its merged weights
 * (into the region of the fine points, unwritten until the resampler runs), stnerf_ray_stop follows it, and after the
 * resampler and the MotionNet-reuse launches of the other layers each flagged layer's fine row list is made by
 * stnerf_visibility_rows (with the layer's grid where it is sample-culled too, in place of stnerf_occupancy_rows); the fine stage
 * walks the lists.  Layer 0 may be flagged (it needs no grid); it is NOT terminated while cache_host is in CAPTURE or REUSE mode
 * (its raw outputs would depend on the performers).  A flagged performer's MotionNet runs fused, as a sample-culled layer's.
 * STNERF_EINVAL before any launch: tau outside [0, 1); params->precision == 2; opacity that differs between the two composites
 * (params->alpha != 1 with l > 2, or a layer_alpha_host entry != 1: the coarse composite ignores them, so its stop depth would
 * be wrong); n1 + n2 > 256 or n > 2^23; misaligned counters.  The workspace grows by n floats (t_stop) and one row list per flagged
 * layer that is not sample-culled: stnerf_render_workspace_bytes_terminated.  visibility_counts_or_null: device, int64 [l][2] =
 * (fine samples tested, not listed) per terminated layer, accumulated. */
int64_t stnerf_render_workspace_bytes_terminated(int64_t n, int l, int n1, int n2, int only_coarse, const int32_t* samples_host,
                                                 const int32_t* terminate_host);
int stnerf_render_rays_terminated(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                                  const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                                  const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                                  float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                                  const stnerf_bkgd_cache* cache_host, const stnerf_layer_rotation* rotations_host,
                                  float* scene_out, const float* layer_alpha_host, const stnerf_occupancy* occupancy_host,
                                  int32_t* counts_or_null, const int32_t* samples_host, int64_t* sample_counts_or_null,
                                  float tau, const int32_t* terminate_host, int64_t* visibility_counts_or_null,
                                  stnerf_stream_t stream);

/* ---- the background's occupancy grid (csrc/sample_rows.hip) ---------------------------------------------
 * Opt-in, inference only: the samples of the background that cross empty cells of a grid over its box get zero outputs instead of
 * a network evaluation.  Not in the reference.  The ray cull's rule "layer 0 cannot carry a grid" stands (a whole-ray cull of a
 * layer that runs on every ray saves nothing); this grid is an argument of its own and culls samples only.
 *   Grid.  A stnerf_occupancy entry as defined above: the same bit layout and the same point-to-cell rule (a NaN coordinate counts
 *   as occupied; subtraction and product separate fp32 operations), 1..256 cells per axis, spanning the axis-aligned fp32 bounds of
 *   the 8 corners of the UNEDITED bkgd_bbox.
 *   Build.  The build above, unchanged: the densities of bkgd_net and bkgd_net_fine at the grid's vertices (through the "fp32"
 *   packs, after bkgd_time_deform_net where it is used), stnerf_occupancy_build with threshold and dilate.
 *   Background sample cull.  In a network stage of ns samples (the coarse stage: n1, the fine stage: n1 + n2) and for EVERY ray
 *   0 .. n-1 -- no mask bit is consulted: the background is evaluated mask or not, evaluated[0] == 2 -- sample k is LISTED when the
 *   point xyz[ray][0][k] lies in an occupied cell or has a NaN coordinate.  That point is the one the background networks would be
 *   given: after layer 0's rotation and un-edit, before bkgd_time_deform_net.  A listed sample is evaluated exactly as without the
 *   cull.  A sample that is not listed gets raw[ray][0][k] = {0, 0, 0, 0}, four exact zero words; no SpaceNet and no MotionNet runs
 *   on it.  Nothing else changes: depths, points, masks, the resampler, the compositor and the scene passes see a `raw` buffer.
 *   With early ray termination on layer 0 a fine sample is listed when it is listed by the grid AND not hidden.
 * stnerf_background_rows makes layer 0's row list of one stage (the row-list contract above): listed = the grid test, and with
 * t_stop not hidden; the rays 0 .. n-1 -- no ray list, no device-side count; xyz / raw (and t) are LAYER 0's slices.
 *   grid_host: mandatory, with bits;
 *   t_or_null / t_stop_or_null: the stage's depths and stnerf_ray_stop's output [n]; t_stop NULL: the grid alone, t is not read;
 *   counts_or_null: device, int64 [2].
 * It also refuses a grid without bits and t_stop without t. */
int stnerf_background_rows(int64_t n, const float* xyz, int64_t xyz_ray_stride, int ns, const stnerf_occupancy* grid_host,
                           const float* t_or_null, int64_t t_ray_stride, const float* t_stop_or_null, float* raw, int64_t raw_ray_stride,
                           int32_t* row_list, int64_t capacity, int32_t* row_count, int64_t* counts_or_null, stnerf_stream_t stream);
/* stnerf_render_rays_terminated with the background's grid.  bkgd_grid_host: one entry (host) or NULL (or bits == NULL) = none,
 * which is what stnerf_render_rays_terminated forwards and which makes exactly the launches it made, in a workspace of
 * stnerf_render_workspace_bytes_terminated.  occupancy_host[0] and samples_host[0] stay refused.  With a grid: stnerf_background_rows
 * on the coarse points after the compaction and on the fine points after the resampler and every MotionNet-reuse launch, each right
 * before its stage, which walks layer 0's row list; only_coarse culls the coarse stage.  Where layer 0's fine stage is terminated
 * the same launch takes t_f / t_stop in place of stnerf_visibility_rows, and the two share layer 0's one row list.  Background
 * cache: a REUSE frame makes no rows launch (layer 0 is in no stage); a CAPTURE frame is culled by the grid and, as ever, not
 * terminated, so the cached raw is the culled one, a function of view and grid only -- the caller keys the cache by the grid.
 * params->precision == 2: STNERF_EINVAL; so are n1 + n2 > 256, n > 2^23 and misaligned counters.
 * stnerf_render_workspace_bytes_background: `background` != 0 = a grid with bits will be given; the workspace grows by layer 0's
 * row list unless termination has given it one.  bkgd_counts_or_null: device, int64 [2] += (samples tested, not listed). */
int64_t stnerf_render_workspace_bytes_background(int64_t n, int l, int n1, int n2, int only_coarse, const int32_t* samples_host,
                                                 const int32_t* terminate_host, int background);
int stnerf_render_rays_background(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                                  const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                                  const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                                  float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                                  const stnerf_bkgd_cache* cache_host, const stnerf_layer_rotation* rotations_host,
                                  float* scene_out, const float* layer_alpha_host, const stnerf_occupancy* occupancy_host,
                                  int32_t* counts_or_null, const int32_t* samples_host, int64_t* sample_counts_or_null,
                                  float tau, const int32_t* terminate_host, int64_t* visibility_counts_or_null,
                                  const stnerf_occupancy* bkgd_grid_host, int64_t* bkgd_counts_or_null, stnerf_stream_t stream);

/* ---- the layer cache (csrc/layer_cache.hip) ---------------------------------------------------------------
 * The background cache's argument holds for every performer: the resampler works per layer, the device RNG is keyed by (seed, global
 * ray index, layer, stream, sample), and a layer's sample points depend on the rays and on that layer's own box, edit, rotation and
 * frame id only.  So layer i's slices of raw_c / raw_f are a function of the view and of layer i's own inputs, whatever the other
 * layers, the opacities, the background's density threshold and the shown flags of the others do.  (params->density_threshold is
 * different with retiming: the coarse composite applies it to the performers before it writes the weights the resampler reads, so a
 * performer's FINE depths, points and raw outputs follow it: it belongs to the caller's key.)  A performer covers a fraction of the view:
 * its cached slices follow its HIT RAYS instead of being dense.  The CALLER decides when "nothing changed" holds and how large
 * an entry must be (stnerf_amd.LayerCache keys and sizes it on the host); the library only moves the data.
 *
 * stnerf_copy_layer_raw_listed is the compact sibling of stnerf_copy_layer_raw: slot j of dense[capacity][ns][4] <-> raw[rays[j]][layer].
 *   to_dense != 0 (capture): ray_list / ray_count = the frame's list of the layer (stnerf_compact_rays; device).  With c = *ray_count:
 *     c <= capacity: *count = c, rays[j] = ray_list[j] and dense[j] = raw[ray_list[j]][layer] for j < c;
 *     c >  capacity: *count = -1 and nothing else is written (so is a c outside 0 .. n, which stnerf_compact_rays never produces).
 *     ray_list may BE rays and ray_count BE count (a second slice captured under the list the first one kept): both stay as they are.
 *   to_dense == 0 (restore): with c = *count: raw[rays[j]][layer] = dense[j] for j < c; a negative c (or one above capacity) copies
 *     nothing.  No other byte of raw is written.  ray_list is not read.  mismatch_or_null: device int64, += 1 when ray_count is given
 *     and *ray_count (the frame's own count) differs from c -- a guard the caller reads only when asked.
 * One wave moves one slot (ns contiguous float4 on both sides), the ray index loaded once per slot, 64-bit indices; a persistent grid
 * of at most 2048 workgroups of 256 strides over the slots and reads the count on the device: no host sync.  HBM-bound: 32 ns + 4
 * bytes per slot.  STNERF_EINVAL before any launch: layer 0 (the background has the dense cache) or >= l, ns < 1, negative capacity,
 * a null pointer, raw / dense not 16-byte aligned, the counter not 8-byte aligned. */
int stnerf_copy_layer_raw_listed(float* raw, int64_t n, int l, int layer, int ns, const int32_t* ray_list, const int32_t* ray_count,
                                 float* dense, int32_t* rays, int32_t* count, int64_t capacity, int to_dense, int64_t* mismatch_or_null,
                                 stnerf_stream_t stream);
/* One layer's entry of the table stnerf_render_rays_layers takes (host struct; every pointer a device pointer).
 *   raw_coarse[capacity][n1][4], raw_fine[capacity][n1+n2][4] (NULL with only_coarse): 16-byte aligned; rays[capacity], count[1].
 *   mode: STNERF_LAYER_CACHE_OFF / _CAPTURE / _REUSE, as the background's modes. */
#define STNERF_LAYER_CACHE_OFF 0
#define STNERF_LAYER_CACHE_CAPTURE 1
#define STNERF_LAYER_CACHE_REUSE 2
typedef struct stnerf_layer_cache {
    float* raw_coarse;
    float* raw_fine;
    int32_t* rays;
    int32_t* count;
    int64_t capacity;
    int32_t mode;
} stnerf_layer_cache;
/* stnerf_render_rays_background with a layer cache.  layers_host: params->l entries (host) or NULL = none, which is what
 * stnerf_render_rays_background forwards; NULL, or every mode OFF, makes exactly the launches that entry made, in a workspace of the
 * same size.  Entry 0 must be OFF (the background keeps its own cache, cache_host; both may be in use in one call); a hidden layer's
 * entry is ignored.  mismatch_or_null: the restore copies' counter, as above.
 *   A layer in REUSE is left out of both network stages (with precision 2: out of both per-network loops); it gets no stand-alone
 *   MotionNet launch and no MotionNet-reuse fill, no ray-bias launch and no row-list launch (the captured slice already holds the
 *   zeros those kernels store).  Its slices are restored where the background's are: the coarse one right after the coarse stage,
 *   before the compositor reads raw_c; the fine one where the fine stage runs, after every MotionNet-reuse launch of the other
 *   layers has read t_c / xyz_c.  Sampler, ray cull, compaction, compositor, resampler and scene passes run for every layer in
 *   every mode, so a REUSE frame is bit-identical to the frame rendered without a cache.
 *   A layer in CAPTURE renders as usual; its slices are copied out after each stage, rays / count written by the coarse copy and
 *   walked by the fine one.
 *   A performer in CAPTURE or REUSE is NOT terminated, exactly as layer 0 under the background cache: its raw outputs would depend
 *   on the other layers otherwise.  (stnerf_amd clears the terminate flag of every shown performer while a layer cache is attached, from
 *   a key's first frame on, so that the uncached, the capture and the reuse frames of a run agree.)
 *   When every evaluated layer comes from a cache no stage is launched at all.
 * Checked on the host before anything is launched: the modes, entry 0, the pointers and their alignment, the capacity. */
int stnerf_render_rays_layers(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                              const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                              const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                              float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                              const stnerf_bkgd_cache* cache_host, const stnerf_layer_rotation* rotations_host,
                              float* scene_out, const float* layer_alpha_host, const stnerf_occupancy* occupancy_host,
                              int32_t* counts_or_null, const int32_t* samples_host, int64_t* sample_counts_or_null,
                              float tau, const int32_t* terminate_host, int64_t* visibility_counts_or_null,
                              const stnerf_occupancy* bkgd_grid_host, int64_t* bkgd_counts_or_null,
                              const stnerf_layer_cache* layers_host, int64_t* mismatch_or_null, stnerf_stream_t stream);

/* ---- depth-tested occluder compositing (csrc/occluder.hip; DESIGN.md sections 4.2 and 7) -----------------------------------------
 * Opt-in, inference only, not in the reference: an element that is NOT a radiance field -- a CG prop, a title card on a plane, a
 * live-action plate with a z-buffer -- put into the scene, hiding what lies behind it and hidden by what lies in front of it.  The
 * scene passes are sums over whole rays and cannot supply that in post; the merged weight of every sample can.
 *   Occluder.  occluder[n][5], fp32 on the device, one row {r, g, b, a, z} per ray of the call.  z is a RAY PARAMETER, in the units
 *   of the depths t the sampler produces (the `depth` output before a caller divides it by far).  a' = a clamped to [0, 1]; a NaN a
 *   counts as 0.  The row is PRESENT when a' > 0 and z is finite, ABSENT otherwise (a' == 0, z NaN, z +-inf).
 *   Front and behind.  Defined for the FINAL stage of the render (fine, or coarse with only_coarse) and one present ray with S samples
 *   per layer: t[l][S] the stage's depths, wM[l][S] its merged weights at source index exactly as stnerf_composite_scene defines
 *   merged_weights, c_k = {r, g, b} the colours the compositor used (sigmoid(rgb), or raw's own with rgb_activated).  Sample k of
 *   layer i is BEHIND when t[i][k] >= z, IN FRONT otherwise; a NaN depth is in front.
 *     front[i][5]  = sum_{k in front} wM {r, g, b, t, 1}          behind[i][5] = the same sum over the samples behind
 *   A layer without network output on the ray (the layers scene_out zeroes: hidden, missed, a grazing hit) gets five exact zeros in
 *   both.  The samples are NOT clipped: a sample that starts in front of z keeps its whole weight, although its interval may reach
 *   behind z (clipping the interval that contains z is out of scope).
 *   Arithmetic: that of scene_out.  Lane j of the ray's wave takes the samples k = j, j + 64, .. ascending, each step acc = acc + w x
 *   with the product and the sum separate fp32 operations, and the five sums go through the same in-place wave scan; the one
 *   difference is that w is replaced by +0.0f on the side the sample does not belong to.  So, bit for bit: a present ray whose z
 *   exceeds every depth has front == scene_out and behind == +0; one whose z is below every depth has behind == scene_out and
 *   front == +0.
 *   Mix, for one present ray; every product, sum and difference is one fp32 operation in the order written:
 *     Af        = ((front[0][4] + front[1][4]) + ..) + front[l-1][4]
 *     T         = 1 - Af where that is > 0, else 0 (a NaN gives 0)
 *     s         = a' T                      q = 1 - a'
 *     pass_i[c] = front_i[c] + q behind_i[c]                        c = 0..4
 *     share     = {s r, s g, s b, s z, s}
 *     occluded_mixed[c] = (((pass_0[c] + pass_1[c]) + ..) + pass_{l-1}[c]) + share[c]
 *   Outputs, {colour(3), depth, acc} as everywhere: occluded_mixed[n][5]; occluded_scene[n][l][5] = pass_i, layer i's share with the
 *   occluder in the scene; occluder_share[n][5] = share, the occluder's own premultiplied share; front_out / behind_out[n][l][5].
 *   On an ABSENT ray occluded_mixed is the bits of mixed_in, occluded_scene and front_out the bits of scene_in, share and behind_out
 *   zeros, and no sample is read.
 * stnerf_scene_occluder: t[n][l][S], raw[n][l][S][4], mask[n][l] (NULL = all set), merged_weights[n][l][S] and params_host
 *   (rgb_activated and evaluated are read) as stnerf_composite_scene took and left them; scene_in[n][l][5] / mixed_in[n][5] its
 *   scene_out / mixed_out.  occluded_mixed is required, the other four outputs may be NULL.  One launch: one wave per ray over a
 *   persistent grid, no LDS; a present ray moves the scene pass's 24 B per sample.  STNERF_EINVAL before any launch: a null input
 *   or occluded_mixed, l outside 1..STNERF_MAX_LAYERS, S < 1, l * S > 65535, raw not 16-byte aligned. */
int stnerf_scene_occluder(const float* t, const float* raw, const uint8_t* mask, const float* merged_weights, int64_t n, int l, int S,
                          const stnerf_composite_params* params_host, const float* scene_in, const float* mixed_in,
                          const float* occluder, float* occluded_mixed, float* occluded_scene, float* occluder_share,
                          float* front_out, float* behind_out, stnerf_stream_t stream);
/*   Occluder stop.  An OPAQUE occluder is also a stop depth of early ray termination: after stnerf_ray_stop,
 *     t_stop[ray] = (present && a' >= 1 && z < t_stop[ray]) ? z : t_stop[ray]
 *   The hidden-sample rule is unchanged (t_f > t_stop), so everything it hides lies behind the occluder and is multiplied by
 *   q = 1 - 1 = +0 in the mix, and the merged weight of a sample in front depends only on samples at or before it and on depths:
 *   with the stop on, occluded_mixed, occluded_scene and occluder_share are BIT-IDENTICAL to the same render with the stop off, on
 *   every ray.  The plain outputs (mixed_fine, layer_fine, scene_out) become those of the terminated scene, as under termination.
 * stnerf_occluder_stop: occluder[n][5], t_stop[n] in place.  One launch, one lane per ray.  STNERF_EINVAL: a null pointer. */
int stnerf_occluder_stop(const float* occluder, int64_t n, float* t_stop, stnerf_stream_t stream);
/* stnerf_render_rays_layers with an occluder.  occluder: [n][5] on the device or NULL = none, which is what stnerf_render_rays_layers
 * forwards (with occluder_stops = 0 and three NULL outputs) and which makes exactly the launches that entry made; the workspace size
 * is the same with or without one.  With an occluder scene_out and occluded_mixed are required (the merged weights exist only with
 * the scene passes); occluded_scene[n][l][5] and occluder_share[n][5] may be NULL.  stnerf_scene_occluder's launch follows the final
 * stage's scene pass on the same stream, while that stage's t, raw and merged weights are live.
 * occluder_stops != 0: stnerf_occluder_stop follows stnerf_ray_stop.  It needs at least one flag of terminate_host set
 * (STNERF_EINVAL otherwise) and is, with only_coarse, the no-op termination is; what termination refuses stays refused (opacity
 * other than 1, precision 2) and what it leaves alone stays alone (layer 0 under the background cache, a cached performer). */
int stnerf_render_rays_occluded(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                                const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                                const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                                float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                                const stnerf_bkgd_cache* cache_host, const stnerf_layer_rotation* rotations_host,
                                float* scene_out, const float* layer_alpha_host, const stnerf_occupancy* occupancy_host,
                                int32_t* counts_or_null, const int32_t* samples_host, int64_t* sample_counts_or_null,
                                float tau, const int32_t* terminate_host, int64_t* visibility_counts_or_null,
                                const stnerf_occupancy* bkgd_grid_host, int64_t* bkgd_counts_or_null,
                                const stnerf_layer_cache* layers_host, int64_t* mismatch_or_null, const float* occluder,
                                int32_t occluder_stops, float* occluded_mixed, float* occluded_scene, float* occluder_share,
                                stnerf_stream_t stream);

/* ---- the render call's optional arguments, stated once ----------------------------------------------------------------------------
 * Every optional argument of stnerf_render_rays_occluded, in that entry's order and with that entry's meaning; the paragraph that
 * introduces an argument above is the field's contract.  A caller sets struct_size = sizeof(stnerf_render_options) and zeroes the
 * rest: an all-zero record with the size set is "no feature" and makes exactly the launches of stnerf_render_rays, in a workspace of
 * stnerf_render_workspace_bytes.  struct_size is what lets a later feature add a FIELD instead of an entry: a size the library does
 * not know is refused with STNERF_EINVAL and a message that names the field, before anything else is looked at.
 * The named entries above are the fixed-argument forms of this call: each fills a record from its arguments and forwards it. */
typedef struct stnerf_render_options {
    int32_t struct_size;                    /* sizeof(stnerf_render_options), set by the caller                                   */
    const stnerf_bkgd_cache* cache;         /* host, or NULL: the background cache (stnerf_render_rays_cached)                      */
    const stnerf_layer_rotation* rot;       /* host, params->l entries, or NULL: per-layer rotations (stnerf_render_rays_rot)       */
    float* scene_out;                       /* device [n][l][5] or NULL: the final stage's scene passes (stnerf_render_rays_scene)  */
    const float* layer_alpha;               /* host, params->l factors finite and >= 0, or NULL (stnerf_render_rays_opacity)        */
    const stnerf_occupancy* occ;            /* host, params->l entries, or NULL: the ray cull's grids (stnerf_render_rays_occupancy)*/
    int32_t* counts;                        /* device int32 [l][2] += (pairs tested, culled), 8-byte aligned, or NULL               */
    const int32_t* samples;                 /* host, params->l flags, or NULL: the sample cull (stnerf_render_rays_samples)         */
    int64_t* sample_counts;                 /* device int64 [l][2] += (samples tested, skipped), or NULL                            */
    float tau;                              /* in [0, 1); read only with a terminate flag set (stnerf_render_rays_terminated)       */
    const int32_t* terminate;               /* host, params->l flags, or NULL: early ray termination of the fine stage              */
    int64_t* visibility_counts;             /* device int64 [l][2] += (fine samples tested, not listed), or NULL                    */
    const stnerf_occupancy* bkgd_grid;      /* host, one entry, or NULL (or bits == NULL): stnerf_render_rays_background            */
    int64_t* bkgd_counts;                   /* device int64 [2] += (samples tested, not listed), or NULL                            */
    const stnerf_layer_cache* layers;       /* host, params->l entries, entry 0 OFF, or NULL (stnerf_render_rays_layers)            */
    int64_t* mismatch;                      /* device int64, the restore copies' counter, or NULL                                   */
    const float* occluder;                  /* device [n][5] or NULL; needs scene_out and occluded_mixed (above)                    */
    int32_t occluder_stops;                 /* != 0: an opaque row lowers the stop depth; needs a terminate flag                    */
    float* occluded_mixed;                  /* device [n][5]; required with an occluder, refused without                            */
    float* occluded_scene;                  /* device [n][l][5] or NULL                                                             */
    float* occluder_share;                  /* device [n][5] or NULL                                                                */
    const uint8_t* bkgd_rays;               /* device uint8 [n] or NULL: the per-ray background mask (below); no named entry         */
} stnerf_render_options;
/* ---- Per-ray background mask (csrc/sample_rows.hip) ------------------------------------------------------
 * Opt-in, inference only, not in the reference: the caller says ray by ray whether layer 0 is evaluated -- what a frame needs whose
 * background comes from another source on some of its rays (a reprojected plate) and from the networks on the others.
 * bkgd_rays: device uint8 [n], one byte per ray of the call; nonzero = evaluate layer 0 on this ray.  NULL: the option is absent.
 *   On a ray whose byte is 0 every sample of layer 0 gets raw = {0, 0, 0, 0}, four exact zero words, in BOTH stages, and no SpaceNet
 *   or MotionNet row: what the background's sample cull does to a sample in an empty cell.  Layer 0's depths and points are made as
 *   ever and take part in the merge as they do there; evaluated[0] stays 2.  On a ray whose byte is nonzero nothing changes.  Rays do
 *   not influence each other, so both statements hold bit for bit.
 *   It composes with the other two culls of layer 0 in the ONE rows launch layer 0 gets per stage: a sample is listed if and only if
 *   its ray's byte is nonzero AND (with a bkgd_grid with bits) its point lies in an occupied cell or has a NaN coordinate AND (with
 *   layer 0's fine stage terminated) !(t > t_stop[ray]).  only_coarse: the coarse stage's rows.
 *   stnerf_render_workspace_bytes_opts: a non-NULL bkgd_rays grows the workspace as a grid with bits does (layer 0's row list).
 *   STNERF_EINVAL before any launch: params->precision == 2; n1 + n2 > 256 or n > 2^23; a background cache (cache->mode) in CAPTURE
 *   or REUSE -- the cached raw would hold the zeros of one mask.  The layer cache is unaffected.
 * stnerf_background_ray_rows makes that row list (the row-list contract above): listed = the ray's flag byte nonzero, and with a
 * grid the grid test, and with t_stop not hidden; the rays 0 .. n-1; stnerf_background_rows' arguments otherwise.
 *   grid_host_or_null may be NULL: no cell test (a grid that is given must have bits);
 *   ray_flags: device uint8 [n], required: a ray whose byte is 0 lists nothing, gets ns zero float4 and loads no point, no depth and
 *   no grid word (the run's 16 flag bytes are loaded once and balloted into a wave-uniform mask).  counts: a masked ray's samples
 *   are both tested and not listed.
 * It also refuses a missing ray_flags, a grid without bits and t_stop without t.  With every byte nonzero and a grid the listed set
 * and the zeros are stnerf_background_rows'. */
int stnerf_background_ray_rows(int64_t n, const float* xyz, int64_t xyz_ray_stride, int ns, const stnerf_occupancy* grid_host_or_null,
                               const float* t_or_null, int64_t t_ray_stride, const float* t_stop_or_null, float* raw,
                               int64_t raw_ray_stride, int32_t* row_list, int64_t capacity, int32_t* row_count,
                               int64_t* counts_or_null, const uint8_t* ray_flags, stnerf_stream_t stream);
/* The workspace of stnerf_render_rays_opts for n rays.  Reads struct_size, samples, terminate, bkgd_grid (a grid with bits grows
 * the workspace as `background` != 0 does above) and bkgd_rays (non-NULL: the same growth); opts_host NULL = an all-zero record =
 * stnerf_render_workspace_bytes. */
int64_t stnerf_render_workspace_bytes_opts(int64_t n, int l, int n1, int n2, int only_coarse, const stnerf_render_options* opts_host);
/* stnerf_render_rays with a record of options; opts_host NULL = no feature.  The one render call with a body: new callers should
 * use this pair. */
int stnerf_render_rays_opts(const float* rays, int64_t n, const float* boxes, int64_t box_ray_stride,
                            const stnerf_nets* nets_host, const stnerf_render_params* params_host, const float* jitter,
                            const float* u, void* workspace, int64_t workspace_bytes, float* mixed_fine,
                            float* mixed_coarse, float* layer_fine, float* layer_coarse, uint8_t* mask,
                            const stnerf_render_options* opts_host, stnerf_stream_t stream);

/* ---- Deep frames (csrc/deep.hip; DESIGN.md sections 4.2 and 7) ---------------------------------------------------------------------
 * Opt-in, inference only, not in the reference: the final stage's merged weights kept as a per-ray list of DEEP SAMPLES, so that any
 * number of depth-tested elements can be composited AFTER the render, with no network (the VFX "deep image").
 *   Kept.  For one ray of the final stage take t[l][S], wM[l][S] and the colour c_k exactly as stnerf_scene_occluder does (the colour
 *   through the compositor's sample edit with its switches off: sigmoid(rgb), or raw's own with rgb_activated).  Sample k of layer i is
 *   KEPT iff !(wM <= w_min), w_min >= 0: the exact zeros of culled, terminated, hidden, missed and grazing samples are dropped, a NaN
 *   weight is kept.  A layer without network output on the ray (the layers scene_out zeroes) has no deep sample.
 *   Segments, per layer, in source order.  merge_dz == 0: every kept sample is its own segment.  merge_dz > 0: t0 = the depth of the
 *   layer's first kept sample on the ray, bin_k = floorf((t_k - t0) / merge_dz), the difference, the quotient and the floor one fp32
 *   operation each; a kept sample STARTS a segment iff it is the layer's first kept sample or bin_k != the previous kept sample's
 *   bin.  The bins are compared as the floats floorf returns -- the same as comparing (int) bin wherever an int holds it -- so a NaN
 *   depth, whose bin is NaN and differs from every bin, opens a segment of its own and ends it.  Segments of different layers may
 *   overlap in depth: wM already carries the layers' mutual occlusion.
 *   Record.  32 bytes, 8 words {r, g, b, a, zw, zf, zb, meta}: {r, g, b, zw, a} = sum of wM {c.r, c.g, c.b, t, 1} over the segment's
 *   kept samples in ascending source index, acc = acc + w x from acc = +0 with the product and the sum separate fp32 operations;
 *   zf, zb = the depths of the segment's first and last kept sample; meta (a uint32 word) = layer | first_k << 8 | count << 16, count
 *   the segment's kept samples.  Hence S <= 256.
 *   Layout.  CSR: offsets[n + 1] int64, samples[total][8] fp32; within a ray layer-major, then source index.  int64 because a frame's
 *   list (1920 x 1080 rays of up to 65535 samples) passes 2^32 records and the offsets are gathered and rebased as tensor indices,
 *   which are int64; 8 bytes per ray are nothing beside 32 per record.  One CALL holds at most 2^31 - 1 records (n l S < 2^31).
 *   The offsets are the ordered exclusive scan of the per-ray counts (csrc/ordered_compact.h's one-workgroup scan of 256-ray block
 *   sums): the layout does not depend on the order in which workgroups run.
 * stnerf_deep_count: counts[n] int32 = the ray's segments.  One wave per ray over a persistent grid; a layer without output is skipped
 *   wave-uniformly, every load of a layer (t and wM, S <= 256: four blocks) is issued before the first is used.
 * stnerf_deep_offsets: counts -> offsets[n + 1]; max_count >= every count (l S), n max_count < 2^31.  workspace: at least
 *   stnerf_deep_workspace_bytes(n) bytes, overwritten; it is NOT part of the render workspace.  Three launches.
 * stnerf_deep_fill: the records of ray r at samples[offsets[r] ..).  A ray with offsets[r + 1] > capacity (or offsets that do not
 *   ascend from >= 0) writes nothing, and no record lands outside [offsets[r], offsets[r + 1]); *deep_total = offsets[n], always: the
 *   caller compares it with capacity, so an overflow is detected and never silent.  The lane that heads a segment sums it.
 * stnerf_deep_composite: elements[n][E][5], 0 <= E <= STNERF_DEEP_MAX_ELEMENTS, rows {r, g, b, a, z} with the occluder's conventions
 *   (a' = clamp(a, 0, 1), a NaN a counts as 0, ABSENT when a' == 0 or z not finite, z a ray parameter).  Per ray the rows are sorted
 *   ascending by z, stable by index, absent rows last; slot j is the j-th row of that order.  P_0 = 1, P_{j+1} = P_j (1 - a'_j).
 *   Deep sample d is BEHIND slot j iff zf_d >= z_j (a NaN zf is in front; samples are not clipped): q_d = P_m, m the number of
 *   present slots d is behind.
 *     pass_i[c]  = sum over layer i's samples of q_d x_d[c],  x = {r, g, b, zw, a}: lane (d mod 64) of the ray's wave, d the sample's
 *                  index in the RAY's list, takes its samples of the layer ascending, acc = acc + q x; the 64 sums go through the
 *                  compositor's in-place wave scan (lanes without a sample of the layer hold +0).  A layer without samples: +0.
 *     Af_j       = sum over ALL samples of the ray of (behind slot j ? +0 : a_d): lane (d mod 64) ascending, then the same scan.
 *     T_j = 1 - Af_j where > 0, else 0 (NaN: 0)     s_j = (a'_j T_j) P_j     share_j = {s r, s g, s b, s z, s}; an absent row: five +0
 *     mixed[c]   = ((((pass_0 + pass_1) + ..) + pass_{l-1}) + share_0) + .. + share_{E-1}, slots in sorted order
 *   mixed_out[n][5]; scene_out[n][l][5] = pass_i or NULL; shares[n][E][5] by the rows' own index, or NULL.  E == 0 is the flatten; a
 *   ray with no deep sample and no present row gives five exact zeros.  One launch, one wave per ray, no LDS.
 * STNERF_EINVAL before any launch: a null pointer that is not optional; l outside 1..STNERF_MAX_LAYERS; S outside 1..256; w_min or
 *   merge_dz negative or NaN; raw or samples not 16-byte aligned; E outside 0..8; capacity < 0; a workspace that is too small. */
#define STNERF_DEEP_MAX_ELEMENTS 8
int64_t stnerf_deep_workspace_bytes(int64_t n);
int stnerf_deep_count(const float* t, const uint8_t* mask, const float* merged_weights, int64_t n, int l, int S,
                      const stnerf_composite_params* params_host, float w_min, float merge_dz, int32_t* counts, stnerf_stream_t stream);
int stnerf_deep_offsets(const int32_t* counts, int64_t n, int64_t max_count, int64_t* offsets, void* workspace, int64_t workspace_bytes,
                        stnerf_stream_t stream);
int stnerf_deep_fill(const float* t, const float* raw, const uint8_t* mask, const float* merged_weights, int64_t n, int l, int S,
                     const stnerf_composite_params* params_host, float w_min, float merge_dz, const int64_t* offsets, float* samples,
                     int64_t capacity, int64_t* deep_total, stnerf_stream_t stream);
int stnerf_deep_composite(const int64_t* offsets, const float* samples, int64_t n, int l, const float* elements, int E, float* mixed_out,
                          float* scene_out, float* shares, stnerf_stream_t stream);
/* The render call with deep output: stnerf_render_options followed by the deep fields.  stnerf_render_rays_opts and
 * stnerf_render_workspace_bytes_opts accept a pointer to either record and tell them apart by struct_size, so every caller of the
 * shorter record -- the named entries among them -- goes on as it was, and an all-zero tail is "no deep output": no new launch, no
 * changed bit, the same render workspace.
 *   deep_samples != NULL turns the feature on.  It needs scene_out (as the occluder does: the merged weights exist only with the scene
 *   passes), deep_offsets, deep_total and deep_workspace, and params->n1 + n2 (n1 with only_coarse) <= 256.  The launches count ->
 *   offsets -> fill follow the final stage's scene pass (and stnerf_scene_occluder if there is one) on the same stream while t, raw
 *   and the merged weights are live; the deep frame is of the scene WITHOUT the occluder.  The render workspace is unchanged.
 *   deep_workspace: stnerf_deep_workspace_bytes(n) + 4 n bytes on the device, 8-byte aligned (the scan's scratch, then the counts). */
typedef struct stnerf_render_options_deep {
    stnerf_render_options base;             /* base.struct_size = sizeof(stnerf_render_options_deep)                                */
    float deep_w_min;                       /* >= 0                                                                                 */
    float deep_merge_dz;                    /* >= 0; 0: every kept sample is a segment                                              */
    int64_t* deep_offsets;                  /* device int64 [n + 1]                                                                 */
    float* deep_samples;                    /* device [deep_capacity][8], 16-byte aligned, or NULL = no deep output                 */
    int64_t deep_capacity;                  /* records deep_samples holds                                                           */
    int64_t* deep_total;                    /* device int64: the records the call needs                                             */
    void* deep_workspace;                   /* device, stnerf_deep_workspace_bytes(n) + 4 n bytes                                   */
} stnerf_render_options_deep;

/* ---- Progressive multi-sample frames (csrc/accumulate.hip): a frame as the per-pixel mean of several
 * passes -- each with its own sub-pixel offset, shutter time and seed -- in which a pixel stops being sampled once its running
 * mean is known well enough.  Three helpers around the render entries, every fp32 operation below on its own (no contraction).
 *
 * Rays of a pixel list: stnerf_generate_rays with two differences.  The pixel of row i is pixels[i] (device int32), or i with
 * pixels = NULL (the contiguous pixels 0..n-1), and
 *     u = (float)(pix % w) + du        v = (float)(pix / w) + dv
 * Every other operation is that kernel's, in its order: with du = dv = 0 row i is bit-identical to row pixels[i] of
 * stnerf_generate_rays.  STNERF_EINVAL before any launch: a null pointer, h or w < 1 or h * w > INT32_MAX, n < 0 or n > h * w (a
 * list names a pixel at most once), a NaN offset, bad frame-id columns.  The kernel leaves the row of a list entry outside
 * [0, h * w) unwritten. */
int stnerf_generate_rays_list(const float* Kinv_host, const float* T_host, int h, int w, const int32_t* pixels, int64_t n, float du,
                              float dv, const float* frame_ids_host, int n_frame_cols, float* rays, int ray_stride,
                              stnerf_stream_t stream);
/* The accumulator.  State per pixel q of P = n_pixels: mean[P][C], m2[P][V] (the first V <= C columns carry a second moment),
 * count[P] int32.  values: n rows of C floats, value_stride floats apart; row i belongs to pixel q = pixels[i], or q = i with
 * pixels = NULL.  For every column x of the row (Welford's update):
 *     c = count[q] + 1
 *     c == 1:  mean = x  (the value itself: one pass reproduces its bits, -0.0 included)          m2 = 0
 *     else:    d = x - mean      mean = mean + d / (float)c      m2 = m2 + d * (x - mean)          (the NEW mean; columns < V)
 *     count[q] = c
 * A list must not name a pixel twice (not checked: the update of a pixel named twice is undefined); an entry outside [0, P) is
 * skipped.  Two launches: one lane per (row, column) reads count, one lane per row then writes it, so no reader races the
 * writer.  HBM-bound: 3 C + 2 V floats per row; no LDS.  STNERF_EINVAL before any launch: a null pointer, V or C out of range
 * (1 <= V <= C <= 4096), value_stride < C, P outside 1..INT32_MAX, n < 0 or n > P. */
int stnerf_accumulate(const float* values, int64_t n, int C, int64_t value_stride, const int32_t* pixels, int64_t n_pixels, int V,
                      float* mean, float* m2, int32_t* count, stnerf_stream_t stream);
/* The pixels still active, in ascending order.  Pixel q is active if and only if
 *     count[q] < min_spp,  or
 *     count[q] < max_spp and, for any of the V columns,  m2[q][v] > tol2 * (float)(count[q] * (count[q] - 1))
 * -- the variance of the mean, m2 / (c (c - 1)), exceeds tol2 = tol^2; the product is the int32 one, converted, times tol2 in
 * fp32 (a NaN m2 is not active).  pixels_out[0 .. *n_out) = the active q ascending (room for P entries); n_out: one device
 * int32.  Deterministic: launch 1 takes the popcount of every 256 pixels with a ballot, launch 2 scans the popcounts in ONE
 * workgroup (1024 per pass), launch 3 writes; no workgroup waits on another.  workspace: device memory of at least
 * stnerf_accumulate_select_workspace_bytes of P (STNERF_EINVAL for P outside 1..INT32_MAX), overwritten.  STNERF_EINVAL before
 * any launch: a null pointer, P or V out of range, not 1 <= min_spp <= max_spp <= 32768, tol2 < 0 or NaN, a workspace too small. */
int64_t stnerf_accumulate_select_workspace_bytes(int64_t n_pixels);
int stnerf_accumulate_select(const float* m2, const int32_t* count, int64_t n_pixels, int V, int min_spp, int max_spp, float tol2,
                             int32_t* pixels_out, int32_t* n_out, void* workspace, int64_t workspace_bytes, stnerf_stream_t stream);

/* ---- A lens model in ray generation (csrc/lens.hip): the rays of a pixel list through a lens that distorts
 * and has an aperture.  Every *, /, + and - below is one IEEE fp32 operation in the order written (no contraction).
 *
 * pix, u, v and the camera vector (cx, cy, cz) = Kinv (u, v, 1) are those of the pixel-list entry above, the skip of a list entry
 * outside [0, h w) included.  Then
 *   distort != 0 -- Brown-Conrady on normalised image coordinates, inverted by a FIXED number of fixed-point rounds (no exit that
 *   depends on the data: a restatement is bit-equal):
 *     xd = cx / cz;  yd = cy / cz;  x = xd;  y = yd;  STNERF_LENS_ITERS rounds of
 *         xx = x*x;  yy = y*y;  xy = x*y;  r2 = xx + yy
 *         rad = ((k3*r2 + k2)*r2 + k1)*r2 + 1.0f
 *         tx  = p1*(xy + xy) + p2*(r2 + (xx + xx))
 *         ty  = p1*(r2 + (yy + yy)) + p2*(xy + xy)
 *         x   = (xd - tx) / rad;   y = (yd - ty) / rad
 *     cx = x * cz;  cy = y * cz                                  (cz is unchanged)
 *   points != NULL -- a thin lens.  The table row is j = phase, or with decorrelate
 *     j = ((hash(pix ^ key) % n_points) + phase) % n_points   in uint32, with the 32-bit mixer
 *     hash: x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16
 *   so that over n_points passes a pixel uses every row exactly once.  (ax, ay) = points[j].  With ax == 0 && ay == 0 the row takes
 *   the pinhole operations and nothing else (a pass through the lens centre is the pinhole ray, bit for bit); otherwise
 *     s = focus / cz;  dx = cx*s - ax;  dy = cy*s - ay;  dz = cz*s;   (cx, cy, cz) = (dx, dy, dz)
 *     o[r] = (T[4r]*ax + T[4r+1]*ay) + T[4r+3]                   r = 0, 1, 2
 *   Without a lens point o[r] = T[4r+3].
 * Normalisation (the squared norm is fmaf(cz, cz, fmaf(cy, cy, cx*cx))), rotation and the frame-id columns are those of the
 * pixel-list entry.  A record with distort == 0 and points == NULL, or lens_host == NULL, IS that entry (the call is forwarded).
 * One lane per row; HBM-bound on the 24 + 4 n_frame_cols bytes a row writes; no LDS.
 * STNERF_EINVAL before any launch: everything the pixel-list entry refuses; a struct_size that is not the size of the record
 * (checked first); with distort a NaN or infinite coefficient; with the lens enabled a third row of Kinv that is not (0, 0, k),
 * k != 0 (the plane in focus and the division by cz assume one cz for the view); with points n_points < 1, phase outside
 * [0, n_points), a focus that is zero, not finite or of the opposite sign to k. */
#define STNERF_LENS_ITERS 20
typedef struct stnerf_lens {
    int32_t struct_size;      /* the size of this record in bytes; anything else: STNERF_EINVAL, checked first */
    int32_t distort;          /* != 0: the five coefficients below are applied */
    float k1, k2, k3, p1, p2; /* Brown-Conrady (the OpenCV order), on normalised image coordinates */
    float focus;              /* camera-space z of the plane in focus; read only with points != NULL */
    const float* points;      /* device [n_points][2]: lens points in camera x, y, world units (already times the aperture radius), or NULL: pinhole */
    int32_t n_points;         /* >= 1 with points */
    int32_t phase;            /* 0 <= phase < n_points: the pass */
    int32_t decorrelate;      /* != 0: every pixel walks the table from its own start */
    uint32_t key;             /* xor-ed into the pixel before hashing */
} stnerf_lens;
int stnerf_generate_rays_lens(const float* Kinv_host, const float* T_host, int h, int w, const int32_t* pixels, int64_t n,
                              float du, float dv, const stnerf_lens* lens_host, const float* frame_ids_host, int n_frame_cols,
                              float* rays, int ray_stride, stnerf_stream_t stream);

/* ---- Reprojection of a key view's rows into a nearby view (csrc/reproject.hip): a forward splat with a depth
 * test, a resolve that turns cracks and silhouettes into holes, and the ascending list of the holes.  Three helpers around the
 * render entries; every *, /, +, - and sqrtf below is one IEEE fp32 operation in the order written (no contraction).
 *
 * Splat.  Row q of a source view (Kinv_s, T_s, h_s, w_s), q = 0..n-1 with n <= h_s w_s, carries a ray parameter t = t_src[q].  The
 * row is absent unless t is finite and t > 0.  (o, d) is the ray of pixel q exactly as stnerf_generate_rays_list gives it with
 * du = dv = 0 (the same device function).  With Wd[12] the world-to-camera 3x4 of the destination pose (the caller inverts T_d in
 * fp64 and rounds to fp32), o_d[3] the destination camera's centre (T_d[4r+3]) and K_d[9] its intrinsics, all row-major:
 *     p[r]   = t * d[r] + o[r]
 *     c[r]   = ((Wd[4r]*p[0] + Wd[4r+1]*p[1]) + Wd[4r+2]*p[2]) + Wd[4r+3]          skipped if  c[2] <= z_min
 *     pix[r] = (K_d[3r]*c[0] + K_d[3r+1]*c[1]) + K_d[3r+2]*c[2]
 *     u = pix[0] / pix[2];  v = pix[1] / pix[2];  iu = (int)rintf(u);  iv = (int)rintf(v)   (pixel centres sit at integers)
 *     skipped if u or v is not finite or (iu, iv) is outside [0, w_d) x [0, h_d)
 *     e[r]   = p[r] - o_d[r];   t' = sqrtf(fmaf(e[2], e[2], fmaf(e[1], e[1], e[0]*e[0])))      (the ray generator's norm order)
 *     key    = ((uint64)bits(t') << 32) | (uint32)(id_base + q);   keys[iv * w_d + iu] = min(keys[..], key)   (a 64-bit atomic)
 * A positive float's bits order as the float does: the nearest surface wins, on an exact tie the lower id, whatever the order of
 * lanes and launches.  The caller fills keys[h_d w_d] with all-ones (= empty) and may splat up to STNERF_REPROJECT_MAX_SOURCES
 * sources into it before resolving; source s uses id_base = n_0 + .. + n_(s-1), and every id stays below 2^31.
 * STNERF_EINVAL before any launch: a null pointer, h w of either view outside 1..INT32_MAX, n < 0 or n > h_s w_s, id_base < 0 or
 * id_base + n > 2^31, z_min not finite or < 0.
 *
 * Resolve.  One lane per destination pixel j.  An empty key is a hole.  Otherwise m = the smallest t' among the non-empty keys of
 * the 3x3 neighbourhood inside the image (j included), and j is a hole as well if  t'_j > m * guard,  guard = 1.0f + rel in fp32:
 * a far surface seen through the cracks of a magnified near one, and the far side of every silhouette, are rendered again.  A filled
 * pixel copies the C floats of row (id - base_s) of its source s (sources_host: n_sources records {values, row_stride, n}, device
 * pointers, base_s as above) to values_out[j][C] and writes t_out[j] = t', src_out[j] = id; a hole gets zeros, a NaN t_out and
 * src_out[j] = -1 (so does a key whose id no record holds).  STNERF_EINVAL before any launch: a null pointer, h_d w_d outside
 * 1..INT32_MAX, C outside 1..64, rel < 0 or NaN, n_sources outside 1..STNERF_REPROJECT_MAX_SOURCES, a record with n < 0 or
 * row_stride < C, n_0 + .. > 2^31 - 1.
 *
 * Hole list.  holes_out[0 .. *n_out) = the j with src[j] < 0, ascending (room for n_pixels entries); n_out: one device int32.  The
 * three launches of stnerf_accumulate_select (csrc/ordered_compact.h), deterministic; workspace as there.  STNERF_EINVAL before any
 * launch: a null pointer, n_pixels outside 1..INT32_MAX, a workspace too small.
 * One lane per row in all three; HBM- and atomics-bound (about 12 B per source row, 4 C + 12 B per destination pixel); no LDS in
 * splat and resolve. */
#define STNERF_REPROJECT_MAX_SOURCES 4
typedef struct stnerf_reproject_source {
    const float* values;  /* device [n][row_stride]: the first C floats of a row are copied */
    int64_t row_stride;   /* floats between rows, >= C */
    int64_t n;            /* rows; the ids of this source are base .. base + n - 1 */
} stnerf_reproject_source;
int stnerf_reproject_splat(const float* Kinv_s_host, const float* T_s_host, int h_s, int w_s, const float* t_src, int64_t n,
                           int64_t id_base, const float* K_d_host, const float* Wd_host, const float* o_d_host, int h_d, int w_d,
                           float z_min, uint64_t* keys, stnerf_stream_t stream);
int stnerf_reproject_resolve(const uint64_t* keys, int h_d, int w_d, float rel, const stnerf_reproject_source* sources_host,
                             int n_sources, int C, float* values_out, float* t_out, int32_t* src_out, stnerf_stream_t stream);
int64_t stnerf_reproject_holes_workspace_bytes(int64_t n_pixels);
int stnerf_reproject_holes(const int32_t* src, int64_t n_pixels, int32_t* holes_out, int32_t* n_out, void* workspace,
                           int64_t workspace_bytes, stnerf_stream_t stream);

/* ---- Adaptive lattice frames (csrc/lattice.hip): render a sparse lattice of pixels, refine the cells whose
 * corners disagree, interpolate the cells whose corners agree.  An approximation, opt-in, inference only.  Every *, + and - below is
 * one IEEE fp32 operation in the order written (no contraction).
 *
 * State of a frame of P = h w pixels, q = y w + x:  values[P][C] (the columns of a packed row; the LAST E of them are exact
 * columns, the first C - E are tested against tol[C - E], a device array) and status[P] uint8: 0 unknown, 1 rendered, 2 filled,
 * 3 queued.  levels = K in 0..4, the top stride S = 2^K.
 *
 * Covered region.  Wc = (w - 1) / S * S,  Hc = (h - 1) / S * S  (integer division).  Wc == 0 or Hc == 0: there is no cell and every
 * pixel is margin.  Otherwise the pixels with x <= Wc and y <= Hc are covered and the others are margin; every cell of every
 * stride s | S with corners on the s-lattice lies inside the covered region.
 *
 * Begin.  status[q] = 3 if q is margin, or force[q] != 0 (force: device uint8[P] or NULL), or x % S == 0 and y % S == 0; else 0.
 *
 * Flat.  A cell (cx, cy, s) has the corners v00 = (cx, cy), v10 = (cx + s, cy), v01 = (cx, cy + s), v11 = (cx + s, cy + s), all of
 * status 1 or 2 (not checked).  It is flat if and only if, for every column c < C - E, the four values are finite and
 * max - min <= tol[c] (one subtraction; a NaN tol[c] is never met), and for every column c >= C - E the four compare equal (==).
 *
 * Classify at stride s (a power of two, 2 <= s <= S; the caller goes s = S, S / 2, .., 2).  Every covered pixel of status 0 looks
 * at the cells of stride s whose closure contains it (one inside a cell, two on an edge, clipped to the covered region).
 *   all of them flat:  status = 2 and, from the FIRST of them (lowest cy, then lowest cx),
 *       fx = (x - cx) / s   gx = 1 - fx   fy = (y - cy) / s   gy = 1 - fy                 (exact: s is a power of two)
 *       top = gx * v00 + fx * v10      bot = gx * v01 + fx * v11      v = gy * top + fy * bot
 *     for every column c < C - E; a column c >= C - E copies v00.
 *   else, x % (s / 2) == 0 and y % (s / 2) == 0:  status = 3.
 *   else it stays 0.
 * Three launches -- a lane per cell writes a flat byte into `flat` (at least (Wc / s) (Hc / s) bytes of device memory; h w always
 * suffices; overwritten), a lane per (pixel, column) fills, a lane per pixel writes the status the fill only read -- so no
 * reader races a writer: a launch reads the values of lattice-s points only, whose status is 1 or 2 and which it never writes, and
 * writes only the pixel it owns.  No atomics, no order dependence.  After s = 2 no covered pixel has status 0.
 *
 * Select.  pixels_out[0 .. *n_out) = the q with status[q] == 3, ascending (room for P entries); n_out: one device int32.  The three
 * launches of stnerf_accumulate_select (csrc/ordered_compact.h), deterministic; workspace as there.
 *
 * Scatter.  Row i of rows (n rows of C floats, row_stride floats apart) becomes values[pixels[i]] and status[pixels[i]] = 1.  An
 * entry outside [0, P) is skipped; a pixel that is not listed is not touched; a list names a pixel at most once (not checked).
 *
 * All kernels are HBM-bound helpers: no LDS beyond the compaction's, no scratch.  STNERF_EINVAL before any launch: a null pointer
 * (force may be NULL; tol may be NULL only if E == C), h or w < 1 or h w > INT32_MAX, levels outside 0..4, s not a power of two in
 * [2, S], not 1 <= C <= 4096 or not 0 <= E <= C, too few flat bytes, row_stride < C, n < 0 or n > P, a workspace too small. */
int stnerf_lattice_begin(int h, int w, int levels, const uint8_t* force, uint8_t* status, stnerf_stream_t stream);
int stnerf_lattice_classify(float* values, uint8_t* status, int h, int w, int C, int E, int levels, int s, const float* tol,
                            uint8_t* flat, int64_t flat_bytes, stnerf_stream_t stream);
int64_t stnerf_lattice_select_workspace_bytes(int64_t n_pixels);
int stnerf_lattice_select(const uint8_t* status, int64_t n_pixels, int32_t* pixels_out, int32_t* n_out, void* workspace,
                          int64_t workspace_bytes, stnerf_stream_t stream);
int stnerf_lattice_scatter(const float* rows, int64_t n, int C, int64_t row_stride, const int32_t* pixels, int64_t n_pixels,
                           float* values, uint8_t* status, stnerf_stream_t stream);

/* ---- Grid proposals (csrc/proposal.hip): a layer's COARSE densities from a grid of vertex densities, no coarse
 * network.  Opt-in, approximate, inference only, not in the reference.  The only thing the final frame takes from the coarse pass is
 * the weights the resampler turns into n2 new depths; a flagged layer's coarse raw slice is a trilinear lookup in its grid, and
 * everything downstream -- the coarse composite, stnerf_ray_stop, the resampler, the fine stage -- is fed with those densities.
 *   Grid.  res = (Rx, Ry, Rz) cells spanning the bounds lo, hi of the layer's UNEDITED box at the layer's frame id, as
 *   stnerf_occupancy states them (inv_a = (float)R_a / (hi_a - lo_a), computed once on the host in fp32).  sigma[Rz+1][Ry+1][Rx+1]
 *   fp32: the density at the vertices, vertex (x, y, z) at (z (Ry + 1) + y) (Rx + 1) + x.
 *   Lookup of point p -- the point the networks would be given: after the ray's rotation and the scale / shift un-edit, before the
 *   MotionNet.  Every line is one fp32 operation (no fused multiply-add).  Per axis a:
 *     d  = p_a - lo_a
 *     g  = d * inv_a
 *     gc = fminf(fmaxf(g, 0), (float)R_a)
 *     i  = (int)fminf(floorf(gc), (float)(R_a - 1))
 *     f  = gc - (float)i
 *     u  = 1 - f
 *   then along x, along y, along z, each lerp as (v0 * u) + (v1 * f): two products and a sum,
 *     c_jk  = (s[z+k][y+j][x] * ux) + (s[z+k][y+j][x+1] * fx)        j, k = 0, 1
 *     c_k   = (c_0k * uy) + (c_1k * fy)
 *     sigma = (c_0 * uz) + (c_1 * fz)
 *   With finite vertex values this form returns the vertex value itself at f = 0 and at f = 1 (v0 + f (v1 - v0) does not).  A point
 *   outside the box clamps to its faces (+-inf included); a NaN coordinate makes fmaxf(g, 0) = 0, so it is carried in by hand: the
 *   sample's sigma is NaN, which is what the network would give it.
 * stnerf_proposal_density: xyz / raw are the LAYER's slices (as in stnerf_stage_layer) with their ray strides in floats.  The rays are
 * the first min(n, *ray_count) slots of ray_list; ray_list == NULL: every ray 0 .. n-1 (layer 0's convention in
 * stnerf_background_rows; ray_count is then not read).  Every sample k < ns of a listed ray gets raw = {0, 0, 0, sigma}, one float4
 * store; a ray that is not listed keeps its bytes.  `layer` names the launch in the profiler record (kernel 20, tag = layer).
 * One launch: one wave per listed ray over a persistent grid, lane (k mod 64) takes samples k, k + 64, ..; the grid record travels
 * by value; eight plain vector loads per sample; no LDS, no scratch.
 * STNERF_EINVAL before any launch: a null pointer (ray_list with ray_count, or neither); sigma not 4-byte, raw not 16-byte aligned or
 * its stride no multiple of 4 floats; res < 1 or (Rx+1)(Ry+1)(Rz+1) >= 2^31; a non-finite lo or inv_cell; ns outside 1..256; layer
 * outside 0..STNERF_MAX_LAYERS-1; n < 0. */
typedef struct stnerf_density_grid {
    const float* sigma;   /* device, [rz+1][ry+1][rx+1] vertex densities, or NULL = this layer has no proposal */
    int32_t res[3];       /* rx, ry, rz >= 1, (rx+1)(ry+1)(rz+1) < 2^31 */
    float lo[3], inv_cell[3];   /* as stnerf_occupancy states them */
} stnerf_density_grid;
int stnerf_proposal_density(const int32_t* ray_list, const int32_t* ray_count, int64_t n, int layer, const float* xyz,
                            int64_t xyz_ray_stride, int ns, const stnerf_density_grid* grid_host, float* raw, int64_t raw_ray_stride,
                            stnerf_stream_t stream);
/* The render call with grid proposals: stnerf_render_options_deep followed by the table.  stnerf_render_rays_opts and
 * stnerf_render_workspace_bytes_opts accept this third record by struct_size exactly as they accept the deep one; the two shorter
 * records and every named entry stay as they are.  proposal: a host table of params->l entries; NULL, or every sigma NULL, is "no
 * feature": no new launch, no changed bit, the same workspace (there is no new workspace with the feature either).
 *   A flagged layer i (proposal[i].sigma != NULL) is in NO coarse network stage, as a layer-cache REUSE layer is in none: no stage
 *   item, no coarse rows launch, no coarse ray-bias, no stand-alone coarse MotionNet.  Its MotionNet-reuse bit is cleared (there are no
 *   moved coarse points to reuse): the fine MotionNet runs fused on all n1 + n2 rows.  Right after the coarse stage and the caches'
 *   copies, one stnerf_proposal_density launch per flagged layer fills its slice of the coarse raw buffer, on the layer's list of hit
 *   rays (layer 0: every ray).  The fine stage, both composites, termination, the scene passes, the occluder and deep output are
 *   untouched; the sample cull of a flagged layer acts on its fine stage only.
 *   Coarse outputs: layer_coarse / mixed_coarse of a flagged layer carry ZERO colour and the grid's depth and alpha.
 *   STNERF_EINVAL: params->precision == 2 (the per-net schedule does not store activated colours); a flagged layer that is hidden or
 *   whose layer cache entry is in CAPTURE / REUSE; layer 0 flagged while the background cache is in CAPTURE / REUSE; layer 0 flagged
 *   together with bkgd_rays or a background grid with bits (the coarse rows launch that stores those zeros is gone: out of scope);
 *   whatever stnerf_proposal_density refuses of a grid; n1 > 256. */
typedef struct stnerf_render_options_proposal {
    stnerf_render_options_deep deep;        /* deep.base.struct_size = sizeof(stnerf_render_options_proposal)                       */
    const stnerf_density_grid* proposal;    /* host, params->l entries, or NULL                                                     */
} stnerf_render_options_proposal;

#ifdef __cplusplus
}
#endif
#endif /* STNERF_H */
