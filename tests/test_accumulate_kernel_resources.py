"""Build-quality gate for the kernels of progressive multi-sample frames (csrc/accumulate.hip), CPU only, in the manner of
tests/test_occluder_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and
the code objects' own metadata is read.

Six helper kernels, all HBM-bound or tiny: generate_rays_list_kernel (one lane per row), accumulate_kernel (one lane per (row,
column): consecutive lanes touch consecutive floats) and accumulate_count_kernel, and the three launches of the ordered
compaction, select_count_kernel / select_scan_kernel / select_write_kernel.  Every one must use no scratch and at most 128 VGPRs
with an occupancy of at least 4 -- the bar of the other helper kernels; the accumulator and the ray generator use no LDS, the
three select kernels a few words of it (the waves' popcounts; the scan's 16 wave sums and its carry).  Measured with hipcc
--offload-arch=gfx950 (ROCm 7.2): the figures are printed."""
import re

import tools.asm_listing as asm

KERNELS = ("generate_rays_list_kernel", "accumulate_kernel", "accumulate_count_kernel", "select_count_kernel", "select_scan_kernel",
           "select_write_kernel")


@asm.needs_hipcc
def test_the_accumulate_kernels_use_no_scratch_and_at_most_128_vgprs():
    kernels = asm.kernels(asm.listing("accumulate.hip"))
    assert len(kernels) == len(KERNELS) and all(sum(k in name for name in kernels) == 1 for k in KERNELS), sorted(kernels)
    for name, k in sorted(kernels.items()):
        asm.assert_no_scratch_no_call(k, name)
        vgprs, scratch, occupancy, lds = k["TotalNumVgprs"], k["ScratchSize"], k["Occupancy"], k["LDSByteSize"]
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
        if "select_" in name:
            assert lds <= 128, (name, lds)
        else:
            assert lds == 0, (name, lds)
    # the definitions' products, quotients and sums stay separate fp32 operations: the file is built without contraction.  That
    # test's check (no fused multiply-add at all) needs one allowance here: a correctly rounded fp32 quotient and square root are
    # themselves EXPANDED into fused operations (the ray generator divides three times and takes one root, the accumulator
    # divides once).  So a probe kernel of one quotient and one of one root are compiled with the same flags, and every kernel
    # must hold exactly the fused operations of its quotients and roots -- one more would be a contracted product of ours.  The ray
    # generator adds the two fmaf it WRITES: the squared norm in torch.norm's order, fmaf(z, z, fmaf(y, y, x x))
    probes = asm.kernels(asm.listing_of(
        "#include <hip/hip_runtime.h>\n"
        "__global__ void probe_div(const float* a, const float* b, float* o) { o[threadIdx.x] = a[threadIdx.x] / b[threadIdx.x]; }\n"
        "__global__ void probe_sqrt(const float* a, float* o) { o[threadIdx.x] = sqrtf(a[threadIdx.x]); }\n", like="accumulate.hip"))

    def fused(kernel):
        body = kernel["body"]
        return (len(re.findall(r"\bv_(?:pk_)?(?:fma|mac|fmac)\w*_f32", body)), len(re.findall(r"\bv_div_fixup_f32", body)),
                len(re.findall(r"\bv_sqrt_f32", body)))
    per_div, one, _ = fused([k for n, k in probes.items() if "probe_div" in n][0])
    per_sqrt, _, one_root = fused([k for n, k in probes.items() if "probe_sqrt" in n][0])
    assert one == 1 and one_root == 1
    expected = {"generate_rays_list_kernel": (3, 1), "accumulate_kernel": (1, 0)}
    for name in sorted(kernels):
        n_fused, n_div, n_sqrt = fused(kernels[name])
        want = next((v for k, v in expected.items() if k in name), (0, 0))
        print(f"{name}: {n_fused} fused operations, {n_div} quotients, {n_sqrt} roots")
        assert (n_div, n_sqrt) == want, (name, n_div, n_sqrt)
        written = 2 if "generate_rays_list_kernel" in name else 0
        assert n_fused == per_div * n_div + per_sqrt * n_sqrt + written, (name, n_fused, per_div, per_sqrt, written)
    from stnerf_amd import build
    assert ("accumulate.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
