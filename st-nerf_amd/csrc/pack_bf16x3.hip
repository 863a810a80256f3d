// The packers of the split-bf16 ("bf16x3") blobs (layouts: mlp_bf16x3.h): the forward blob of a network from host tensors
// (stnerf_pack_net_bf16x3) or device tensors (stnerf_pack_net_bf16x3_device), and the backward chain's blob of transposed weights
// (stnerf_pack_dx_bf16x3_device).  A blob is stated once, as a table of passes; bx_pack_element() is one element of one pass and
// holds the only fp32 -> three-bf16 split outside the kernels' own split8.  The host entry runs it in a CPU loop, the device entries
// in a grid-stride kernel (blockIdx.y = the pass): a test of the host blob is a test of the table the device entry packs with
// (tests/test_bf16x3_pack_cpu.py; host == device, bit for bit: tests/test_gpu_backward.py,
// test_device_packer_writes_the_host_packers_blob).
//
// Reference: modeling/spacenet.py:16-160, modeling/motion_net.py:7-71.
#include <math.h>
#include <string.h>

#include "mlp_bf16x3.h"

namespace stnerf {

struct BxPackPass {
    const float* src;
    int64_t dst;        // stream passes: byte offset of the pass in the blob; copies: float offset in the blob
    int32_t in, n0, ksteps;
    int32_t mode;       // 0 hidden, 1 staged encoding (limit `lim`), 2 stage2.0 (256 hidden columns, then PE(pos)), 3 plain copy of `ksteps` floats,
                        // 4 TRANSPOSED (the backward chain's A operands): output n = n0 + 32 fb + c is COLUMN n of src (valid below `lim`),
                        //   K index k = bx_kmap_hidden(..) is its ROW (valid below `klim`)
    int32_t lim;
    int32_t klim, nblk; // nblk (read in every stream mode): feature blocks per K step -- 4; a half pass of the backward chain: 2
};
struct BxPackTable {
    BxPackPass pass[32];
    int32_t count;
};

// fp32 -> three bf16 pieces, x = p0 + p1 + p2: integer round-to-nearest-even on the bit pattern at every step (inf / NaN: as is),
// one exact fp32 subtraction per piece -- the same bits on either side.
__host__ __device__ inline uint32_t bx_bf16_rne(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7f800000u) == 0x7f800000u) return u >> 16;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__host__ __device__ inline void bx_split3(float w, uint32_t (&p)[3]) {
    p[0] = bx_bf16_rne(w);
    const float r1 = w - __builtin_bit_cast(float, p[0] << 16);
    p[1] = bx_bf16_rne(r1);
    const float r2 = r1 - __builtin_bit_cast(float, p[1] << 16);
    p[2] = bx_bf16_rne(r2);
}

__host__ __device__ inline int bx_pass_elements(const BxPackPass& ps) { return ps.mode == 3 ? ps.ksteps : ps.ksteps * ps.nblk * 512; }
// Element e of a pass.  A copy: one float.  A stream pass: the three pieces of B position (K step tt, lane, j) of feature block fb,
// [K step][feature block][piece][lane][8 bf16]; zero where the position has no input column (padding).
__host__ __device__ inline void bx_pack_element(const BxPackPass& ps, char* blob, int e) {
    if (ps.mode == 3) {
        reinterpret_cast<float*>(blob)[ps.dst + e] = ps.src[e];
        return;
    }
    const int j = e & 7, lane = (e >> 3) & 63, fb = (e >> 9) % ps.nblk, tt = (e >> 9) / ps.nblk;
    const int h = lane >> 5, n = ps.n0 + 32 * fb + (lane & 31);
    int64_t at = -1;   // index of the weight in src
    if (ps.mode == 4) {
        const int k = bx_kmap_hidden(tt, h, j);
        if (k < ps.klim && n < ps.lim) at = (int64_t)k * ps.in + n;
    } else {
        int k;
        if (ps.mode == 0 || (ps.mode == 2 && tt < 16)) {
            k = bx_kmap_hidden(tt, h, j);
        } else {
            k = bx_kmap_enc(ps.mode == 2 ? tt - 16 : tt, h, j);
            k = k < ps.lim ? (ps.mode == 2 ? 256 + k : k) : -1;
        }
        if (k >= 0) at = (int64_t)n * ps.in + k;
    }
    uint32_t p[3] = {0, 0, 0};
    if (at >= 0) bx_split3(ps.src[at], p);
    uint16_t* u = reinterpret_cast<uint16_t*>(blob + ps.dst) + (size_t)(tt * ps.nblk + fb) * (BX_UNIT / 2) + lane * 8 + j;
    u[0] = (uint16_t)p[0];
    u[BX_CHUNK / 2] = (uint16_t)p[1];
    u[BX_CHUNK] = (uint16_t)p[2];
}
__global__ void pack_bf16x3_device_kernel(BxPackTable t, char* blob) {
    const BxPackPass ps = t.pass[blockIdx.y];
    const int total = bx_pass_elements(ps);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) bx_pack_element(ps, blob, e);
}

// Consts and stream of a network's forward blob (the tensor count is checked by the f32 section's packer); `who` names the entry.
static int bx_pack_table(const char* who, int kind, const float* const* W, const float* const* B, const BxLayout& X, BxPackTable& t) {
    memset(&t, 0, sizeof(t));
    int64_t off = X.stream_off;
    auto pass = [&](const float* w, int in, int n0, int ksteps, int mode, int lim) {
        t.pass[t.count++] = BxPackPass{w, off, in, n0, ksteps, mode, lim, 0, 4};
        off += (int64_t)ksteps * 4 * BX_UNIT;
    };
    auto cpy = [&](const float* src, int count, int cst_off) { t.pass[t.count++] = BxPackPass{src, X.consts_off / 4 + cst_off, 0, 0, count, 3, 0, 0, 4}; };
    if (STNERF_NET_IS_SPACE(kind)) {
        const bool deep = STNERF_NET_IS_DEEP(kind);
        const int nt = deep ? 12 : 10;
        const int in_f[7] = {63, 256, 256, 256, 319, 256, 256};
        for (int i = 0; i < 7; ++i) cpy(B[i], 256, BXC_B + 256 * i);
        for (int i = 0; i < 2 && deep; ++i) cpy(B[9 + i], 128, BXC_B_DEEP + 128 * i);
        cpy(W[7], 256, BXC_W_SIGMA);
        cpy(W[nt - 1], 3 * 128, BXC_W_RGB2);
        for (int i = 0; i < 7; ++i)
            for (int half = 0; half < 2; ++half) {
                if (i == 0)
                    pass(W[0], 63, 128 * half, 4, 1, 63);
                else if (i == 4)   // stage2.0: the 256 features, then PE(pos)
                    pass(W[4], 319, 128 * half, 20, 2, 63);
                else
                    pass(W[i], in_f[i], 128 * half, 16, 0, 0);
            }
        // rgb_net.1: the 256 backbone columns (direction / time columns: mlp_raybias.hip)
        pass(W[8], 256 + 27 + (STNERF_NET_USES_TIME(kind) ? 21 : 0), 0, 16, 0, 0);
        for (int i = 0; i < 2 && deep; ++i) pass(W[9 + i], 128, 0, 8, 0, 0);
    } else {
        for (int i = 0; i < 5; ++i) cpy(B[i], 128, BXM_B + 128 * i);
        cpy(W[5], 3 * 128, BXM_W_OUT);
        pass(W[0], 84, 0, 6, 1, 84);
        for (int i = 1; i < 5; ++i) pass(W[i], 128, 0, 8, 0, 0);
    }
    STNERF_REQUIRE(off == X.total_bytes && t.count <= 32, "%s: internal: stream of %lld B, expected %lld", who, (long long)(off - X.stream_off),
                   (long long)X.n_slots * BX_SLOT);
    return STNERF_OK;
}

}  // namespace stnerf

using namespace stnerf;

extern "C" int64_t stnerf_packed_bytes_bf16x3(int kind) {
    if (!STNERF_NET_IS_SPACE(kind) && kind != STNERF_NET_MOTION) {
        set_error("packed_bytes_bf16x3: unknown net kind %d", kind);
        return STNERF_EINVAL;
    }
    return bx_layout(kind).total_bytes;
}

// Host: tensors and destination in host memory.
extern "C" int stnerf_pack_net_bf16x3(int kind, const float* const* W, const float* const* B, int n_tensors, void* dst_host,
                                      int64_t dst_bytes) {
    STNERF_REQUIRE(W && B && dst_host, "pack_net_bf16x3: null pointer");
    STNERF_REQUIRE(STNERF_NET_IS_SPACE(kind) || kind == STNERF_NET_MOTION, "pack_net_bf16x3: unknown net kind %d", kind);
    const BxLayout X = bx_layout(kind);
    STNERF_REQUIRE(dst_bytes >= X.total_bytes, "pack_net_bf16x3: dst too small (%lld < %lld)", (long long)dst_bytes, (long long)X.total_bytes);
    memset(dst_host, 0, (size_t)X.total_bytes);
    // ---- the f32 section = the exact-f32 blob (also validates the tensor count)
    if (const int rc = stnerf_pack_net(kind, W, B, n_tensors, dst_host, X.f32_floats * 4)) return rc;
    // The split x = x0 + x1 + x2 is exact for finite values up to bf16's largest finite number, 0x7f7f = 3.3895e38; above it (fp32's
    // last 0.4 %) the leading piece rounds to inf and x0 + x1 is inf - inf; an inf or NaN weight would likewise turn every output
    // it touches into NaN where ATen propagates the inf.  Refused here rather than silently different: the f32 section holds
    // every weight and bias of the network.
    {
        const float* f = static_cast<const float*>(dst_host);
        for (int64_t i = 0; i < X.f32_floats; ++i)
            STNERF_REQUIRE(fabsf(f[i]) <= 3.3895313892515355e38f, "pack_net_bf16x3: a weight or bias is not finite or exceeds bf16's range "
                           "(|w| <= 3.3895e38): %g -- use the exact-f32 packing (stnerf_pack_net) for such a network", (double)f[i]);
    }
    BxPackTable t;
    if (const int rc = bx_pack_table("pack_net_bf16x3", kind, W, B, X, t)) return rc;
    for (int s = 0; s < t.count; ++s) {
        const int n = bx_pass_elements(t.pass[s]);
        for (int e = 0; e < n; ++e) bx_pack_element(t.pass[s], static_cast<char*>(dst_host), e);
    }
    return STNERF_OK;
}

// Device: the same blob from tensors in DEVICE memory (training: the weights change with every optimizer step): the f32 section by
// stnerf_pack_net_device, consts and stream by one launch.  No finiteness check here (no host round trip): an inf / NaN / > 3.39e38
// weight gives NaN pieces and NaN outputs, which a training loop notices; stnerf_pack_net_bf16x3 is the one that refuses.
extern "C" int stnerf_pack_net_bf16x3_device(int kind, const float* const* W, const float* const* B, int n_tensors, void* dst_dev,
                                             int64_t dst_bytes, stnerf_stream_t stream) {
    STNERF_REQUIRE(W && B && dst_dev, "pack_net_bf16x3_device: null pointer");
    STNERF_REQUIRE(STNERF_NET_IS_SPACE(kind) || kind == STNERF_NET_MOTION, "pack_net_bf16x3_device: unknown net kind %d", kind);
    const BxLayout X = bx_layout(kind);
    STNERF_REQUIRE(dst_bytes >= X.total_bytes, "pack_net_bf16x3_device: dst too small (%lld < %lld)", (long long)dst_bytes, (long long)X.total_bytes);
    STNERF_REQUIRE(((uintptr_t)dst_dev & 1023) == 0, "pack_net_bf16x3_device: the blob must be 1 KB aligned");
    // ---- the f32 section (also validates the tensor count), then the pad and the consts cleared
    if (const int rc = stnerf_pack_net_device(kind, W, B, n_tensors, dst_dev, X.f32_floats * 4, stream)) return rc;
    if (hipMemsetAsync(static_cast<char*>(dst_dev) + X.f32_floats * 4, 0, (size_t)(X.stream_off - X.f32_floats * 4), as_stream(stream)) != hipSuccess)
        return STNERF_ELAUNCH;
    BxPackTable t;
    if (const int rc = bx_pack_table("pack_net_bf16x3_device", kind, W, B, X, t)) return rc;
    hipLaunchKernelGGL(pack_bf16x3_device_kernel, dim3(32, t.count), dim3(256), 0, as_stream(stream), t, static_cast<char*>(dst_dev));
    STNERF_CHECK_LAUNCH("pack_net_bf16x3_device");
    return STNERF_OK;
}

// The backward chain's blob (train_space_dx_bx_kernel): [consts: density_net.0's 256 weights | the colour head [3][128] | pad to 4 KB]
// [stream: the transposed weights as bf16 triples in consumption order, 24 KB slots].  with_dpos: with the two half passes that
// carry the gradient on to PE(pos) (stage2.0's PE columns behind its first pass, stage1.0 at the end) -- a stream without them for
// networks whose sample points need no gradient.  Tensors as for stnerf_pack_net_device (reference layout, fused-path networks:
// TKERNEL_INC_RAW, USE_DIR, no deep_rgb).
extern "C" int64_t stnerf_packed_bytes_dx_bf16x3(int kind, int with_dpos) {
    if (kind != STNERF_NET_SPACE && kind != STNERF_NET_SPACE_TIME) {
        set_error("packed_bytes_dx_bf16x3: kind %d (SpaceNets without deep_rgb)", kind);
        return STNERF_EINVAL;
    }
    return (int64_t)BXD_CONST * 4 + (int64_t)bxd_slots(with_dpos != 0) * BX_SLOT;
}

extern "C" int stnerf_pack_dx_bf16x3_device(int kind, const float* const* W, int n_tensors, int with_dpos, void* dst_dev, int64_t dst_bytes,
                                            stnerf_stream_t stream) {
    STNERF_REQUIRE(W && dst_dev, "pack_dx_bf16x3_device: null pointer");
    const int64_t total = stnerf_packed_bytes_dx_bf16x3(kind, with_dpos);
    if (total < 0) return (int)total;
    STNERF_REQUIRE(n_tensors == 10, "pack_dx_bf16x3_device: a SpaceNet without deep_rgb has 10 weight tensors, got %d", n_tensors);
    for (int i = 0; i < 10; ++i) STNERF_REQUIRE(W[i], "pack_dx_bf16x3_device: tensor %d is null", i);
    STNERF_REQUIRE(dst_bytes >= total && ((uintptr_t)dst_dev & 1023) == 0, "pack_dx_bf16x3_device: the destination needs %lld bytes, 1 KB aligned",
                   (long long)total);
    if (hipMemsetAsync(dst_dev, 0, (size_t)BXD_CONST * 4, as_stream(stream)) != hipSuccess) return STNERF_ELAUNCH;
    BxPackTable t;
    memset(&t, 0, sizeof(t));
    int64_t off = (int64_t)BXD_CONST * 4;
    auto pass = [&](const float* w, int in, int n0, int ksteps, int nlim, int klim, int nblk) {
        t.pass[t.count++] = BxPackPass{w, off, in, n0, ksteps, 4, nlim, klim, nblk};
        off += (int64_t)ksteps * nblk * BX_UNIT;
    };
    t.pass[t.count++] = BxPackPass{W[7], BXD_W_SIGMA, 0, 0, 256, 3, 0, 0, 4};
    t.pass[t.count++] = BxPackPass{W[9], BXD_W_RGB2, 0, 0, 3 * 128, 3, 0, 0, 4};
    const int in8 = 256 + 27 + (kind == STNERF_NET_SPACE_TIME ? 21 : 0);
    for (int half = 0; half < 2; ++half) pass(W[8], in8, 128 * half, 8, 256, 128, 4);          // rgb_net.1[:, :256]
    for (int l = 6; l >= 1; --l) {
        const int in = l == 4 ? 319 : 256;
        pass(W[l], in, 0, 16, 256, 256, 4);
        if (l == 4 && with_dpos) pass(W[4], 319, 256, 16, 319, 256, 2);                        // stage2.0's PE(pos) columns: a half pass
        pass(W[l], in, 128, 16, 256, 256, 4);
    }
    if (with_dpos) pass(W[0], 63, 0, 16, 63, 256, 2);                                          // stage1.0: a half pass
    STNERF_REQUIRE(off == total && t.count <= 32, "pack_dx_bf16x3_device: internal: %lld B, expected %lld", (long long)off, (long long)total);
    hipLaunchKernelGGL(pack_bf16x3_device_kernel, dim3(32, t.count), dim3(256), 0, as_stream(stream), t, static_cast<char*>(dst_dev));
    STNERF_CHECK_LAUNCH("pack_dx_bf16x3_device");
    return STNERF_OK;
}
