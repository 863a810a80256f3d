"""Build-quality gate for the two kernels of occluder compositing (csrc/occluder.hip: scene_occluder_kernel,
occluder_stop_kernel), CPU only, in the manner of tests/test_termination_kernel_resources.py: hipcc cross-compiles the file to
gfx950 assembly with the flags the build gives it, and the code objects' own metadata is read.

scene_occluder_kernel is layer_scene_kernel with two sets of sums: HBM-bound, launched with __launch_bounds__(256) over a
persistent grid, every load of a layer (three blocks of t, wM and the raw float4) in flight before the first use, ten accumulators
and the mix in registers.  Both kernels must use no scratch and no LDS and at most 128 VGPRs -- room for four workgroups per CU,
the bar of the other helper kernels.  Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): scene_occluder_kernel 72 VGPRs,
occupancy 7; occluder_stop_kernel 4 VGPRs, occupancy 8."""
import re

import tools.asm_listing as asm


@asm.needs_hipcc
def test_the_occluder_kernels_use_no_scratch_and_at_most_128_vgprs():
    text = asm.listing("occluder.hip")
    kernels = asm.kernels(text)
    assert sorted(k for k in kernels if "scene_occluder_kernel" in k or "occluder_stop_kernel" in k) == sorted(kernels) and len(kernels) == 2
    for name, k in sorted(kernels.items()):
        asm.assert_no_scratch_no_call(k, name)
        vgprs, scratch, occupancy, lds = k["TotalNumVgprs"], k["ScratchSize"], k["Occupancy"], k["LDSByteSize"]
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
    # the definitions' products and sums stay separate fp32 operations: the file is built without contraction
    assert not re.search(r"\bv_(pk_)?(fma|mac|fmac)\w*_f32", text)
    from stnerf_amd import build
    assert ("occluder.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
