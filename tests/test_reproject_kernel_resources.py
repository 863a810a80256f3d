"""Build-quality gate for the kernels of reprojection into a nearby view (csrc/reproject.hip), CPU only, in the manner of
tests/test_accumulate_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and
the code objects' own metadata is read.

Five helper kernels: reproject_splat_kernel (one lane per source row, one 64-bit atomic), reproject_resolve_kernel (one lane per
destination pixel) and the three launches of the ordered compaction shared with csrc/accumulate.hip (csrc/ordered_compact.h),
select_count_kernel / select_scan_kernel / select_write_kernel.  Every one must use no scratch and at most 128 VGPRs with an
occupancy of at least 4 -- the bar of the other helper kernels; splat and resolve declare no LDS and use none, the three select
kernels a few words of it (the waves' popcounts; the scan's 16 wave sums and its carry).  Measured with hipcc
--offload-arch=gfx950 (ROCm 7.2): the figures are printed."""
import re

import tools.asm_listing as asm

KERNELS = ("reproject_splat_kernel", "reproject_resolve_kernel", "select_count_kernel", "select_scan_kernel", "select_write_kernel")


@asm.needs_hipcc
def test_the_reproject_kernels_use_no_scratch_and_at_most_128_vgprs():
    kernels = asm.kernels(asm.listing("reproject.hip"))
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
    # the depth test is ONE 64-bit vector atomic minimum, and only the splat holds it
    body = lambda k: [v["body"] for n, v in kernels.items() if k in n][0]
    assert len(re.findall(r"\bglobal_atomic_umin_x2\b", body("reproject_splat_kernel"))) == 1
    assert all("atomic" not in body(k) for k in KERNELS[1:])
    # the definitions' products, quotients and sums stay separate fp32 operations: the file is built without contraction.  A
    # correctly rounded fp32 quotient and square root are themselves EXPANDED into fused operations, so a probe kernel of one
    # quotient and one of one root are compiled with the same flags, and every kernel must hold exactly the fused operations of
    # its quotients and roots plus the fmaf it WRITES -- one more would be a contracted product of ours.  The splat divides five
    # times (the ray's three, u and v), takes two roots (the ray's norm, t') and writes four fmaf (the two squared norms, in the
    # ray generator's order); the resolve and the compaction hold none.
    probes = asm.kernels(asm.listing_of(
        "#include <hip/hip_runtime.h>\n"
        "__global__ void probe_div(const float* a, const float* b, float* o) { o[threadIdx.x] = a[threadIdx.x] / b[threadIdx.x]; }\n"
        "__global__ void probe_sqrt(const float* a, float* o) { o[threadIdx.x] = sqrtf(a[threadIdx.x]); }\n", like="reproject.hip"))

    def fused(kernel):
        b = kernel["body"]
        return (len(re.findall(r"\bv_(?:pk_)?(?:fma|mac|fmac)\w*_f32", b)), len(re.findall(r"\bv_div_fixup_f32", b)),
                len(re.findall(r"\bv_sqrt_f32", b)))
    per_div, one, _ = fused([k for n, k in probes.items() if "probe_div" in n][0])
    per_sqrt, _, one_root = fused([k for n, k in probes.items() if "probe_sqrt" in n][0])
    assert one == 1 and one_root == 1
    expected = {"reproject_splat_kernel": (5, 2, 4)}
    for name in sorted(kernels):
        n_fused, n_div, n_sqrt = fused(kernels[name])
        n_want_div, n_want_sqrt, written = next((v for k, v in expected.items() if k in name), (0, 0, 0))
        print(f"{name}: {n_fused} fused operations, {n_div} quotients, {n_sqrt} roots")
        assert (n_div, n_sqrt) == (n_want_div, n_want_sqrt), (name, n_div, n_sqrt)
        assert n_fused == per_div * n_div + per_sqrt * n_sqrt + written, (name, n_fused, per_div, per_sqrt, written)
    from stnerf_amd import build
    assert ("reproject.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
