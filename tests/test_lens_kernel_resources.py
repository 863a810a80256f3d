"""Build-quality gate for the kernel of the lens model in ray generation (csrc/lens.hip), CPU only, in the manner of
tests/test_accumulate_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and
the code object's own metadata is read.

One helper kernel, generate_rays_lens_kernel (one lane per row, HBM-bound on the row it writes).  It must use no scratch, at most
128 VGPRs with an occupancy of at least 4 -- the bar of the other helper kernels -- and no LDS.  Measured with hipcc
--offload-arch=gfx950 (ROCm 7.2): the figures are printed."""
import re

import tools.asm_listing as asm

KERNELS = ("generate_rays_lens_kernel",)


@asm.needs_hipcc
def test_the_lens_kernel_uses_no_scratch_no_lds_and_at_most_128_vgprs():
    kernels = asm.kernels(asm.listing("lens.hip"))
    assert len(kernels) == len(KERNELS) and all(sum(k in name for name in kernels) == 1 for k in KERNELS), sorted(kernels)
    for name, k in sorted(kernels.items()):
        asm.assert_no_scratch_no_call(k, name)
        vgprs, scratch, occupancy, lds = k["TotalNumVgprs"], k["ScratchSize"], k["Occupancy"], k["LDSByteSize"]
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
        assert lds == 0, (name, lds)
    # the definition's products, quotients and sums stay separate fp32 operations: the file is built without contraction.  A
    # correctly rounded fp32 quotient and square root are themselves EXPANDED into fused operations, so a probe kernel of one
    # quotient and one of one root are compiled with the same flags, and the kernel must hold exactly the fused operations of its
    # quotients and roots plus the two fmaf it WRITES (the squared norm in torch.norm's order) -- one more would be a contracted
    # product of ours.  Quotients in the listing: xd, yd, the round's two (the loop is not unrolled), focus / cz, the norm's three.
    probes = asm.kernels(asm.listing_of(
        "#include <hip/hip_runtime.h>\n"
        "__global__ void probe_div(const float* a, const float* b, float* o) { o[threadIdx.x] = a[threadIdx.x] / b[threadIdx.x]; }\n"
        "__global__ void probe_sqrt(const float* a, float* o) { o[threadIdx.x] = sqrtf(a[threadIdx.x]); }\n", like="lens.hip"))

    def fused(kernel):
        body = kernel["body"]
        return (len(re.findall(r"\bv_(?:pk_)?(?:fma|mac|fmac)\w*_f32", body)), len(re.findall(r"\bv_div_fixup_f32", body)),
                len(re.findall(r"\bv_sqrt_f32", body)))
    per_div, one, _ = fused([k for n, k in probes.items() if "probe_div" in n][0])
    per_sqrt, _, one_root = fused([k for n, k in probes.items() if "probe_sqrt" in n][0])
    assert one == 1 and one_root == 1
    for name in sorted(kernels):
        n_fused, n_div, n_sqrt = fused(kernels[name])
        print(f"{name}: {n_fused} fused operations, {n_div} quotients, {n_sqrt} roots")
        assert (n_div, n_sqrt) == (8, 1), (name, n_div, n_sqrt)
        assert n_fused == per_div * n_div + per_sqrt * n_sqrt + 2, (name, n_fused, per_div, per_sqrt)
    from stnerf_amd import build
    assert ("lens.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
