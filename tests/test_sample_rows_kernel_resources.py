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
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def _metadata(text):
    """{symbol: {field: value}} from the ``amdhsa.kernels`` records of an assembly listing, plus ``TotalNumVgprs``, ``ScratchSize``,
    ``Occupancy`` and ``LDSByteSize`` from the summary the compiler prints behind each kernel."""
    records = text[text.index("amdhsa.kernels:"):]
    out = {}
    for rec in re.split(r"\n  - ", records)[1:]:
        named = re.search(r"\n    \.name:\s+(\S+)", rec)          # (the record's own fields sit four columns in, its arguments' deeper)
        if named is None:
            continue                                             # (the entries of amdhsa.version behind the kernels)
        out[named.group(1)] = {f: int(re.search(r"\n    \." + f + r":\s+(\d+)", rec).group(1)) for f in FIELDS
                               if re.search(r"\n    \." + f + r":", rec)}
    for name, fields in out.items():
        summary = text[text.index("\n" + name + ":"):]
        body = summary[:summary.index("s_endpgm")]
        assert "scratch_" not in body and "s_swappc" not in body, name
        for key in ("TotalNumVgprs", "ScratchSize", "Occupancy", "LDSByteSize"):
            fields[key] = int(re.search(r"; " + key + r": (\d+)", summary).group(1))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="no hipcc")
def test_the_sample_rows_kernel_uses_no_scratch_no_lds_and_at_most_128_vgprs(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "sample_rows.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "sample_rows.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    kernels = _metadata(open(asm).read())
    # NC 1 / 2 / 4 x (ray list and grid: 1; ray list and t_stop, with or without a grid: 2; every ray and grid, with or without
    # t_stop: 2; per-ray mask, with or without a grid, with or without t_stop: 4)
    assert len(kernels) == 27 and all("sample_rows_kernel" in k for k in kernels), sorted(kernels)
    for name, m in sorted(kernels.items()):
        registers = m["vgpr_count"] + m.get("agpr_count", 0)
        derived = min(8, 512 // max(8, (registers + 7) // 8 * 8))
        print(f"{name}: {m['vgpr_count']} VGPRs + {m.get('agpr_count', 0)} AGPRs, scratch {m['private_segment_fixed_size']}, "
              f"LDS {m['group_segment_fixed_size']}, occupancy {m['Occupancy']} (derived {derived})")
        assert m["private_segment_fixed_size"] == 0 and m["ScratchSize"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0 and m["LDSByteSize"] == 0, (name, m)
        assert registers <= 128 and m["TotalNumVgprs"] <= 128, (name, m)
        assert m["Occupancy"] >= 4 and derived >= 4, (name, m)
