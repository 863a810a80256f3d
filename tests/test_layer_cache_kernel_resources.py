"""Build-quality gate for the listed copy (csrc/layer_cache.hip: copy_layer_raw_listed_kernel), CPU only, in the manner of
tests/test_termination_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it,
and the code objects' own metadata is read.

The kernel is a copy: one wave per slot, four slots in flight per wave, launched with __launch_bounds__(256).  It is HBM-bound and
hides latency with resident waves, so both flavours (capture, restore) must use no scratch -- the four slots' addresses and values
are indexed by compile-time constants and live in registers --, no LDS, and at most 128 VGPRs (four workgroups per CU at least)."""
import tools.asm_listing as asm


@asm.needs_hipcc
def test_the_listed_copy_kernels_use_no_scratch_and_at_most_128_vgprs():
    text = asm.listing("layer_cache.hip")
    kernels = asm.kernels(text)
    assert len(kernels) == 2 and all("copy_layer_raw_listed_kernel" in k for k in kernels), sorted(kernels)   # capture, restore
    for name, k in sorted(kernels.items()):
        asm.assert_no_scratch_no_call(k, name)
        vgprs, scratch, occupancy, lds = k["TotalNumVgprs"], k["ScratchSize"], k["Occupancy"], k["LDSByteSize"]
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
    # a slot's samples move as 16-byte vectors
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
