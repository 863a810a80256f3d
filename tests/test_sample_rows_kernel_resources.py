"""Build-quality gate for the rows kernel (csrc/sample_rows.hip: sample_rows_kernel, the one kernel behind occupancy_rows,
visibility_rows, background_rows and background_ray_rows), CPU only: hipcc cross-compiles the file to gfx950 with the flags the build
gives it and the code objects' own METADATA is read -- the ``amdhsa.kernels`` records (.vgpr_count, .agpr_count,
.private_segment_fixed_size, .group_segment_fixed_size) and the compiler's per-kernel summary (TotalNumVgprs, ScratchSize, Occupancy,
LDSByteSize).

The kernel is launched with __launch_bounds__(256): four waves, one per SIMD of a CU.  It is a latency-bound walk over HBM (the
point, depth and grid-word loads), so it must leave room for at least FOUR workgroups per CU -- at most 128 VGPRs -- and use no
scratch (every ballot of a run is indexed by compile-time constants and lives in registers) and no LDS.  The occupancy is also
derived from the register count: a gfx950 SIMD holds 512 registers per lane, allocated in granules of 8, and at most 8 waves.
Measured with hipcc --offload-arch=gfx950 (ROCm 7.2) over the 27 kernels: 22 .. 46 VGPRs and occupancy 7 or 8 as the compiler
reports it, but for the four gridded NC = 2 kernels without a ray list: 88 .. 94 VGPRs, occupancy 5 (the ballots of a run sit in
scalar registers).  No AGPRs."""
import tools.asm_listing as asm


@asm.needs_hipcc
def test_the_sample_rows_kernel_uses_no_scratch_no_lds_and_at_most_128_vgprs():
    kernels = asm.kernels(asm.listing("sample_rows.hip"))
    # NC 1 / 2 / 4 x (ray list and grid: 1; ray list and t_stop, with or without a grid: 2; every ray and grid, with or without
    # t_stop: 2; per-ray mask, with or without a grid, with or without t_stop: 4)
    assert len(kernels) == 27 and all("sample_rows_kernel" in k for k in kernels), sorted(kernels)
    for name, m in sorted(kernels.items()):
        asm.assert_no_scratch_no_call(m, name)
        registers = m["vgpr_count"] + m["agpr_count"]
        derived = min(8, 512 // max(8, (registers + 7) // 8 * 8))
        print(f"{name}: {m['vgpr_count']} VGPRs + {m['agpr_count']} AGPRs, scratch {m['private_segment_fixed_size']}, "
              f"LDS {m['group_segment_fixed_size']}, occupancy {m['Occupancy']} (derived {derived})")
        resources = {k: v for k, v in m.items() if k != "body"}
        assert m["private_segment_fixed_size"] == 0 and m["ScratchSize"] == 0, (name, resources)
        assert m["group_segment_fixed_size"] == 0 and m["LDSByteSize"] == 0, (name, resources)
        assert registers <= 128 and m["TotalNumVgprs"] <= 128, (name, resources)
        assert m["Occupancy"] >= 4 and derived >= 4, (name, resources)
