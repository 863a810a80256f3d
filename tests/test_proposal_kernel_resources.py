"""Build-quality gate for the lookup kernel of the grid proposals (csrc/proposal.hip), CPU only, in the manner of
tests/test_deep_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and the code
object's own metadata is read -- register counts, scratch and LDS, nothing else.

proposal_density_kernel gathers eight vertices per sample and is bound by those loads: it wants every wave slot, so at most 128
VGPRs (four waves per SIMD), no scratch, no spills and no LDS.  Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): 70 VGPRs
(the sample loop is unrolled twice), occupancy 7."""
import tools.asm_listing as asm


@asm.needs_hipcc
def test_the_lookup_kernel_uses_no_scratch_no_spills_no_lds_and_at_most_128_vgprs():
    kernels = asm.kernels(asm.listing("proposal.hip"))
    assert len(kernels) == 1 and "proposal_density_kernel" in next(iter(kernels)), sorted(kernels)
    for name, k in kernels.items():
        asm.assert_no_scratch_no_call(k, name)
        vgprs, scratch, occupancy, lds = k["TotalNumVgprs"], k["ScratchSize"], k["Occupancy"], k["LDSByteSize"]
        vspill, sspill = k["vgpr_spill_count"], k["sgpr_spill_count"]
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}, spills {vspill} / {sspill}")
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert lds == 0, (name, lds)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
    body = next(iter(kernels.values()))["body"]
    assert "v_fma_f32" not in body and "v_fmac_f32" not in body and "v_pk_fma_f32" not in body      # every product and sum on its own
    assert "global_store_dwordx4" in body                                                          # one float4 store per sample
    from stnerf_amd import build
    assert ("proposal.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
