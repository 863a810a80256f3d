"""Build-quality gate for the kernel of early ray termination (csrc/termination.hip: ray_stop_kernel; the rows kernel of
stnerf_visibility_rows is gated by tests/test_sample_rows_kernel_resources.py), CPU only, in the manner of
tests/test_sample_cull_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and
the code objects' own metadata is read.

The kernel is launched with __launch_bounds__(256): four waves, one per SIMD of a CU.  It is a latency-bound walk over HBM (the
merge's dependent loads), so it must leave room for at least FOUR workgroups per CU -- occupancy >= 4 waves per SIMD, i.e. at most
128 VGPRs -- and use no scratch: every per-layer array of the merge (cursors, head depths) is indexed by compile-time constants and
lives in registers.
Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): ray_stop_kernel<4 | 8 | 16>: 34 / 58 / 106 VGPRs, occupancy 8 / 8 / 4."""
import tools.asm_listing as asm


@asm.needs_hipcc
def test_the_termination_kernels_use_no_scratch_and_fit_four_workgroups_per_cu():
    kernels = asm.kernels(asm.listing("termination.hip"))
    assert len(kernels) == 3 and all("ray_stop_kernel" in k for k in kernels), sorted(kernels)       # LCAP 4 / 8 / 16
    for name, k in sorted(kernels.items()):
        asm.assert_no_scratch_no_call(k, name)
        vgprs, scratch, occupancy, lds = k["TotalNumVgprs"], k["ScratchSize"], k["Occupancy"], k["LDSByteSize"]
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
