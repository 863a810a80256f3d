"""Build-quality gate for the row-list flavours of the stage kernels (csrc/mlp_wave_rows.hip, csrc/mlp_bf16x3_rows.hip: the kernel
text of csrc/mlp_wave_stage_kernel.h / csrc/mlp_bf16x3_stage_kernel.h under a name of its own, with the row-list locate step), CPU
only: hipcc cross-compiles them to gfx950 assembly, next to the files of the kernels they are flavours of.  In the manner of
tests/test_kernel_resources.py, which pins those parents and passes unchanged: its patterns must not match the new symbols.

The flavours may cost no register and (almost) no vector instruction over their parents: the packed word (ray << 8 | k) REPLACES the
division and the ray-list load of the locate step.  Measured with hipcc --offload-arch=gfx950 (ROCm 7.2), vector instructions as
listed in the work-item loop, parent -> row-list flavour:
    exact f32:   3160 -> 3180,  deep_rgb 3536 -> 3546;   split bf16: 11951 -> 11968,  deep_rgb 12787 -> 12803
The listing holds BOTH locate paths of the flavour (a launch mixes listed and unlisted layers) and an item runs one of them, so the
difference as listed, 10 .. 20 instructions, bounds what an item can pay from above; the ceiling below is 32 (1 % of the exact-f32
loop, 0.3 % of the split-bf16 one).  Registers: 392 / 476 and 496 / 496 VGPRs + AGPRs, the parents' counts; no scratch."""
import re
from concurrent.futures import ThreadPoolExecutor

import tools.asm_listing as asm

MARGIN = 32          # vector instructions as listed in the work-item loop, over the parent flavour

# the patterns of tests/test_kernel_resources.py
PARENT = {"mlp_wave": r"_ZN6stnerf21mlp_wave_stage_kernelILb[01]E\S*", "mlp_bf16x3": r"_ZN6stnerf23mlp_bf16x3_stage_kernelILb[01]E\S*"}
ROWS = {"mlp_wave": r"_ZN6stnerf26mlp_wave_stage_rows_kernelILb[01]E\S*", "mlp_bf16x3": r"_ZN6stnerf28mlp_bf16x3_stage_rows_kernelILb[01]E\S*"}


def _flavours(kernels, pattern):
    """{deep_rgb: (vector instructions as listed in the work-item loop, VGPRs + AGPRs, scratch bytes, occupancy, MFMAs)} of the inference
    instantiations (the training tap's is not a parent of a row-list flavour)."""
    out = {}
    for name, k in kernels.items():
        if not re.fullmatch(pattern, name) or "StoreTapArgs" in name:
            continue
        lines = k["body"].split("\n")
        loop = next(i for i, l in enumerate(lines) if "This Loop Header: Depth=1" in l)
        ops = [l.split()[0] for l in lines[loop:] if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))]
        vec = sum(1 for o in ops if o.startswith("v_") and "mfma" not in o)
        asm.assert_no_scratch_no_call(k, name)
        out["ILb1E" in name] = (vec, k["TotalNumVgprs"], k["ScratchSize"], k["Occupancy"], k["body"].count("v_mfma"))
    return out


@asm.needs_hipcc
def test_row_list_flavours_cost_no_register_and_no_scratch():
    sources = ["mlp_bf16x3.hip", "mlp_bf16x3_rows.hip", "mlp_wave.hip", "mlp_wave_rows.hip"]
    with ThreadPoolExecutor(len(sources)) as pool:          # (side by side; what another gate of this run compiled is not compiled again)
        texts = dict(zip(sources, pool.map(asm.listing, sources)))
    for stem in ("mlp_wave", "mlp_bf16x3"):
        parent_text, rows_text = texts[stem + ".hip"], texts[stem + "_rows.hip"]
        parent_kernels, rows_kernels = asm.kernels(parent_text), asm.kernels(rows_text)
        # a name of their own, in a file of their own: the parents' patterns see three kernels where they saw three, and none here
        assert sum(bool(re.fullmatch(PARENT[stem], n)) for n in parent_kernels) == 3
        assert not re.findall(PARENT[stem], rows_text) and not re.findall(ROWS[stem], parent_text)
        assert sum(bool(re.fullmatch(ROWS[stem], n)) for n in rows_kernels) == 2
        assert [k["ScratchSize"] for k in rows_kernels.values()] == [0, 0]          # nothing else in the file
        parent, rows = _flavours(parent_kernels, PARENT[stem]), _flavours(rows_kernels, ROWS[stem])
        assert sorted(parent) == sorted(rows) == [False, True]
        for deep in (False, True):
            (pv, pr, _, _, pm), (rv, rr, rs, ro, rm) = parent[deep], rows[deep]
            print(f"{stem} deep_rgb={deep}: vector instructions as listed {pv} -> {rv}, registers {pr} -> {rr}")
            assert rs == 0 and ro == 1, (stem, deep, rs, ro)                    # no scratch, one wave per SIMD
            assert rr <= pr and rr <= 512, (stem, deep, rr, pr)                 # no more registers than the parent flavour
            assert rm == pm, (stem, deep, rm, pm)                               # the same MFMAs
            assert rv <= pv + MARGIN, f"{stem} deep_rgb={deep}: {rv} vector instructions in the work-item loop, parent {pv} (+{MARGIN} allowed)"
