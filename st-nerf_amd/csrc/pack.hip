// The packers of the exact-f32 networks -- host (stnerf_pack_net) and device (stnerf_pack_net_device): the reference's
// nn.Linear tensors -> the [K/4][N][4] blob the MFMA kernels stream their A operands from (layouts: mlp_common.h) -- the
// transposed sections of the fused backward chains (stnerf_pack_transposed), and the stand-alone positional encoding.
// (The split-bf16 blobs: pack_bf16x3.hip.)
//
// Reference: modeling/spacenet.py:16-160, modeling/motion_net.py:7-71, utils/dimension_kernel.py:3-73.
#include <stdlib.h>
#include <string.h>

#include "mlp_common.h"

namespace stnerf {

// ---------------------------------------------------------------------------------------------
// Stand-alone positional encoding (op-level API; the MLP kernels encode their inputs themselves)
// ---------------------------------------------------------------------------------------------
__global__ void encode_kernel(const float* __restrict__ x, int64_t n, int dim, int n_freq, int include_input,
                              float* __restrict__ y) {
    const int out_dim = dim * (include_input + 2 * n_freq);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one thread per output element
    if (e >= n * out_dim) return;
    const int64_t row = e / out_dim;
    int f = (int)(e - row * out_dim);
    const float* xr = x + row * dim;
    if (include_input) {
        if (f < dim) {
            y[e] = xr[f];
            return;
        }
        f -= dim;
    }
    const int fq = f / (2 * dim), w = f - fq * 2 * dim;
    const int d = w % dim;
    float sn, cs;
    sincos_pe(xr[d] * (float)(1 << fq), sn, cs);
    y[e] = w < dim ? sn : cs;
}

// ---------------------------------------------------------------------------------------------
// The blob of a network, stated once: a table of segments, each either a linear layer's re-blocking -- (out, in) row-major ->
// [ceil(in / 4) (padded to kq)][out][4], zero padded -- or a plain copy.  pack_table() lists the segments of a network kind;
// pack_element() is one output float of one segment.  The host packer runs it in a CPU loop, the device packer in a grid-stride
// kernel (blockIdx.y = the segment): one layout, and a test of the host blob is a test of the table both use.
// ---------------------------------------------------------------------------------------------
struct PackSeg {
    const float* src;
    int64_t dst_off;   // floats
    int32_t n, in_f, kq;   // kq > 0: W[n][in_f] -> [kq][n][4];  kq == 0: copy `n` floats
};
struct PackTable {
    PackSeg seg[26];
    int32_t count;
    int64_t total;     // floats of the blob
};
__host__ __device__ inline int64_t pack_seg_floats(const PackSeg& sg) { return sg.kq > 0 ? (int64_t)sg.kq * sg.n * 4 : sg.n; }
__host__ __device__ inline float pack_element(const PackSeg& sg, int64_t i) {
    if (sg.kq == 0) return sg.src[i];
    const int r = (int)(i & 3);
    const int64_t q = i >> 2;
    const int n = (int)(q % sg.n), k = 4 * (int)(q / sg.n) + r;
    return k < sg.in_f ? sg.src[(int64_t)n * sg.in_f + k] : 0.f;
}
__global__ void pack_net_device_kernel(PackTable t, float* dst) {
    const PackSeg sg = t.seg[blockIdx.y];
    const int64_t total = pack_seg_floats(sg);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        dst[sg.dst_off + i] = pack_element(sg, i);
}

// The segments of a network (tensors in the reference's order; checks their count, not the pointers: each entry does that in its
// own order); `who` names the entry in the error texts.
static int pack_table(const char* who, int kind, const float* const* W, const float* const* B, int n_tensors, PackTable& t) {
    memset(&t, 0, sizeof(t));
    auto lin = [&](const float* w, int n, int in_f, int kq, int64_t off) { t.seg[t.count++] = PackSeg{w, off, n, in_f, kq}; };
    auto cpy = [&](const float* src, int count, int64_t off) { t.seg[t.count++] = PackSeg{src, off, count, 0, 0}; };
    if (STNERF_NET_IS_SPACE(kind)) {
        const bool ut = STNERF_NET_USES_TIME(kind), deep = STNERF_NET_IS_DEEP(kind);
        const SpaceLayout L = space_layout(ut, deep);
        const int nt = deep ? 12 : 10;
        STNERF_REQUIRE(n_tensors == nt, "%s: this SpaceNet kind takes %d tensors, got %d", who, nt, n_tensors);
        t.total = L.total;
        const int in_f[7] = {63, 256, 256, 256, 319, 256, 256};
        for (int i = 0; i < 7; ++i) {
            lin(W[i], 256, in_f[i], L.kq[i], L.w[i]);
            cpy(B[i], 256, L.b[i]);
        }
        cpy(W[7], 256, L.w_sigma);
        cpy(B[7], 1, L.b_sigma);
        lin(W[8], 128, 256 + 27 + (ut ? 21 : 0), L.kq_rgb1, L.w_rgb1);
        cpy(B[8], 128, L.b_rgb1);
        for (int i = 0; i < 2 && deep; ++i) {
            lin(W[9 + i], 128, 128, 32, L.w_deep[i]);
            cpy(B[9 + i], 128, L.b_deep[i]);
        }
        cpy(W[nt - 1], 3 * 128, L.w_rgb2);
        cpy(B[nt - 1], 3, L.b_rgb2);
    } else if (kind == STNERF_NET_MOTION) {
        const MotionLayout L = motion_layout();
        STNERF_REQUIRE(n_tensors == 6, "%s: MotionNet takes 6 tensors, got %d", who, n_tensors);
        t.total = L.total;
        const int in_f[5] = {84, 128, 128, 128, 128};
        for (int i = 0; i < 5; ++i) {
            lin(W[i], 128, in_f[i], L.kq[i], L.w[i]);
            cpy(B[i], 128, L.b[i]);
        }
        cpy(W[5], 3 * 128, L.w_out);
        cpy(B[5], 3, L.b_out);
    } else {
        set_error("%s: unknown net kind %d", who, kind);
        return STNERF_EINVAL;
    }
    return STNERF_OK;
}

}  // namespace stnerf

using namespace stnerf;

extern "C" int64_t stnerf_packed_bytes(int kind) {
    switch (kind) {
        case STNERF_NET_SPACE: return space_layout(false).total * 4;
        case STNERF_NET_SPACE_TIME: return space_layout(true).total * 4;
        case STNERF_NET_SPACE_DEEP: return space_layout(false, true).total * 4;
        case STNERF_NET_SPACE_TIME_DEEP: return space_layout(true, true).total * 4;
        case STNERF_NET_MOTION: return motion_layout().total * 4;
        default: set_error("packed_bytes: unknown net kind %d", kind); return STNERF_EINVAL;
    }
}

// Host: tensors and destination in host memory.
extern "C" int stnerf_pack_net(int kind, const float* const* W, const float* const* B, int n_tensors, void* dst_host,
                               int64_t dst_bytes) {
    STNERF_REQUIRE(W && B && dst_host, "pack_net: null pointer");
    PackTable t;
    if (const int rc = pack_table("pack_net", kind, W, B, n_tensors, t)) return rc;
    STNERF_REQUIRE(dst_bytes >= t.total * 4, "pack_net: dst too small");
    for (int i = 0; i < n_tensors; ++i) STNERF_REQUIRE(W[i] && B[i], "pack_net: tensor %d is null", i);
    float* dst = static_cast<float*>(dst_host);
    memset(dst, 0, (size_t)t.total * 4);   // (the pads between the sections)
    for (int s = 0; s < t.count; ++s) {
        const PackSeg& sg = t.seg[s];
        const int64_t n = pack_seg_floats(sg);
        for (int64_t i = 0; i < n; ++i) dst[sg.dst_off + i] = pack_element(sg, i);
    }
    return STNERF_OK;
}

// Device: the same blob from tensors that live in HBM -- what a training loop needs after every optimizer.step() (the host packer
// costs a D2H of the weights, a CPU loop and an H2D per network: 165 ms per iteration for the eight networks of a C3 model against
// 40 ms of kernels).  One launch per network.
extern "C" int stnerf_pack_net_device(int kind, const float* const* W, const float* const* B, int n_tensors, void* dst_dev, int64_t dst_bytes,
                                      stnerf_stream_t stream) {
    STNERF_REQUIRE(W && B && dst_dev, "pack_net_device: null pointer");
    PackTable t;
    if (const int rc = pack_table("pack_net_device", kind, W, B, n_tensors, t)) return rc;
    for (int i = 0; i < n_tensors; ++i) STNERF_REQUIRE(W[i] && B[i], "pack_net_device: tensor %d is null", i);
    STNERF_REQUIRE(dst_bytes >= t.total * 4, "pack_net_device: dst too small");
    if (hipMemsetAsync(dst_dev, 0, (size_t)t.total * 4, as_stream(stream)) != hipSuccess) return STNERF_ELAUNCH;
    hipLaunchKernelGGL(pack_net_device_kernel, dim3(64, t.count), dim3(256), 0, as_stream(stream), t, static_cast<float*>(dst_dev));
    STNERF_CHECK_LAUNCH("pack_net_device");
    return STNERF_OK;
}

// The transposed sections the fused backward chains read (csrc/train_wave.hip): out x in (row stride ldw) -> [out / 4][n_pad][4], zero
// for the padded inputs; n_pad == 0: a plain copy of out * in floats (the heads).  One launch for a network: blockIdx.y = section.
namespace stnerf {
struct TransposeTable {
    stnerf_transpose_section seg[12];
};
__global__ void pack_transposed_kernel(TransposeTable t, float* dst) {
    const stnerf_transpose_section sg = t.seg[blockIdx.y];
    const int64_t total = sg.n_pad > 0 ? (int64_t)sg.n_out * sg.n_pad : (int64_t)sg.n_out * sg.n_in;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        float v;
        if (sg.n_pad > 0) {
            const int r = (int)(i & 3);
            const int64_t q = i >> 2;
            const int n = (int)(q % sg.n_pad), o = 4 * (int)(q / sg.n_pad) + r;
            v = n < sg.n_in ? sg.w[(int64_t)o * sg.ldw + n] : 0.f;
        } else {
            v = sg.w[(i / sg.n_in) * sg.ldw + (i % sg.n_in)];
        }
        dst[sg.dst_off + i] = v;
    }
}
}  // namespace stnerf

extern "C" int stnerf_pack_transposed(const stnerf_transpose_section* sections, int count, float* dst_dev, int64_t dst_floats, stnerf_stream_t stream) {
    STNERF_REQUIRE(sections && dst_dev && count >= 1 && count <= 12, "pack_transposed: 1 .. 12 sections");
    TransposeTable t;
    memset(&t, 0, sizeof(t));
    for (int i = 0; i < count; ++i) {
        const stnerf_transpose_section& q = sections[i];
        STNERF_REQUIRE(q.w && q.n_out >= 1 && q.n_in >= 1 && q.ldw >= q.n_in && q.dst_off >= 0, "pack_transposed: bad section %d", i);
        STNERF_REQUIRE(q.n_pad == 0 || ((q.n_out & 3) == 0 && q.n_pad >= q.n_in), "pack_transposed: section %d: out %% 4 == 0 and n_pad >= in", i);
        const int64_t floats = q.n_pad > 0 ? (int64_t)q.n_out * q.n_pad : (int64_t)q.n_out * q.n_in;
        STNERF_REQUIRE(q.dst_off + floats <= dst_floats, "pack_transposed: section %d ends beyond the destination", i);
        t.seg[i] = q;
    }
    hipLaunchKernelGGL(pack_transposed_kernel, dim3(64, count), dim3(256), 0, as_stream(stream), t, dst_dev);
    STNERF_CHECK_LAUNCH("pack_transposed");
    return STNERF_OK;
}

extern "C" int stnerf_encode(const float* x, int64_t n, int dim, int n_freq, int include_input, float* y,
                             stnerf_stream_t stream) {
    STNERF_REQUIRE(x && y, "encode: null pointer");
    STNERF_REQUIRE(n >= 0 && dim >= 1 && n_freq >= 0 && n_freq <= 30 && (include_input == 0 || include_input == 1),
                   "encode: bad shape n=%lld dim=%d n_freq=%d", (long long)n, dim, n_freq);
    const int64_t tot = n * dim * (include_input + 2 * n_freq);
    if (tot == 0) return STNERF_OK;
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, as_stream(stream), x, n, dim,
                       n_freq, include_input, y);
    STNERF_CHECK_LAUNCH("encode");
    return STNERF_OK;
}
