"""Build-quality gate for the kernels of deep frames (csrc/deep.hip), CPU only, in the manner of
tests/test_occluder_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and the
code objects' own metadata is read -- register counts, scratch and LDS, nothing else.

deep_ray_kernel<false> (count) and <true> (fill) walk a ray alike: a layer's t and wM in four blocks in flight before the first
use, ballots for the segment starts; deep_composite_kernel keeps eight sorted rows, their prefix products and eight Af partial sums in
registers.  All must use no scratch and at most 128 VGPRs -- room for four workgroups per CU, the bar of the other helper kernels --
and no LDS beyond the few words the offset scan's workgroups exchange.  Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): count 19
VGPRs, fill 83, composite 103, the three scan kernels 6 / 26 / 26 with 16 / 68 / 16 bytes of LDS."""
import tools.asm_listing as asm


@asm.needs_hipcc
def test_the_deep_kernels_use_no_scratch_and_at_most_128_vgprs():
    kernels = asm.kernels(asm.listing("deep.hip"))
    ray = sorted(k for k in kernels if "deep_ray_kernel" in k)
    composite = [k for k in kernels if "deep_composite_kernel" in k]
    scan = [k for k in kernels if "deep_block_sum_kernel" in k or "select_scan_kernel" in k or "deep_offsets_kernel" in k]
    assert len(ray) == 2 and len(composite) == 1 and len(scan) == 3 and len(kernels) == 6, sorted(kernels)
    for name, k in sorted(kernels.items()):
        asm.assert_no_scratch_no_call(k, name)
        vgprs, scratch, occupancy, lds = k["TotalNumVgprs"], k["ScratchSize"], k["Occupancy"], k["LDSByteSize"]
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
        assert lds == 0 if name in ray + composite else lds <= 128, (name, lds)      # only the scan's workgroups exchange words
    from stnerf_amd import build
    assert ("deep.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
