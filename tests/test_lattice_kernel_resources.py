"""Build-quality gate for the kernels of adaptive lattice frames (csrc/lattice.hip), CPU only, in the manner of
tests/test_accumulate_kernel_resources.py: hipcc cross-compiles the file to gfx950 with the flags the build gives it, and only the
code objects' own metadata is read -- the resource summary the compiler writes for every kernel; no instruction is looked at.

Eight helper kernels, all HBM-bound or tiny: lattice_begin_kernel and lattice_mark_kernel (one lane per pixel),
lattice_flat_kernel (one lane per cell), lattice_fill_kernel and lattice_scatter_kernel (one lane per (pixel, column):
consecutive lanes touch consecutive floats), and the three launches of the ordered compaction, select_count_kernel /
select_scan_kernel / select_write_kernel.  Every one must use no scratch and at most 128 VGPRs with an occupancy of at least 4 --
the bar of the other helper kernels; the five lattice kernels use no LDS, the three select kernels a few words of it (the waves'
popcounts; the scan's 16 wave sums and its carry).  Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): the figures are
printed."""
import tools.asm_listing as asm

KERNELS = ("lattice_begin_kernel", "lattice_flat_kernel", "lattice_fill_kernel", "lattice_mark_kernel", "lattice_scatter_kernel",
           "select_count_kernel", "select_scan_kernel", "select_write_kernel")
FLAGS = ["-ffp-contract=off"]


@asm.needs_hipcc
def test_the_lattice_kernels_use_no_scratch_and_at_most_128_vgprs():
    kernels = asm.kernels(asm.listing("lattice.hip"))
    assert len(kernels) == len(KERNELS) and all(sum(k in name for name in kernels) == 1 for k in KERNELS), sorted(kernels)
    for name, k in sorted(kernels.items()):
        vgprs, scratch, occupancy, lds = k["TotalNumVgprs"], k["ScratchSize"], k["Occupancy"], k["LDSByteSize"]
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
        if "select_" in name:
            assert lds <= 128, (name, lds)
        else:
            assert lds == 0, (name, lds)


def test_the_build_compiles_the_file_without_contraction():
    from stnerf_amd import build
    assert ("lattice.hip", FLAGS) in [(s, f) for s, f in build.SOURCES]
