"""Build-quality gate for the per-ray mask's rows kernel (csrc/background_rays.hip: background_ray_rows_kernel), CPU only, in the
manner of tests/test_background_grid_kernel_resources.py: hipcc cross-compiles the file to gfx950 with the flags the build gives it
and the code objects' own METADATA is read -- the ``amdhsa.kernels`` records (.vgpr_count, .agpr_count, .private_segment_fixed_size,
.group_segment_fixed_size) and the compiler's per-kernel summary (Occupancy, ScratchSize).  No instruction is looked at.

The bounds are the sibling's, for the sibling's reason: a latency-bound walk over HBM launched with __launch_bounds__(256) must leave
room for at least FOUR workgroups per CU -- at most 128 VGPRs -- and use no scratch (every ballot of a run is indexed by compile-time
constants and lives in registers) and no LDS.  The occupancy is also derived from the register count: a gfx950 SIMD holds 512
registers per lane, allocated in granules of 8, and at most 8 waves.
Measured with hipcc --offload-arch=gfx950 (ROCm 7.2), background_ray_rows_kernel<NC = 1 | 2 | 4> over (grid, t_stop) = (no, no) /
(no, yes) / (yes, no) / (yes, yes): 33 / 38 / 41 / 46, 22 / 26 / 90 / 94 and 23 / 25 / 29 / 33 VGPRs, no AGPRs; occupancy 7 as the
compiler reports it, 5 for the two gridded NC = 2 kernels (the ballots of a run sit in scalar registers)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def _metadata(text):
    """{symbol: {field: value}} from the ``amdhsa.kernels`` records of an assembly listing, plus ``Occupancy`` and ``ScratchSize``
    from the summary the compiler prints behind each kernel."""
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
        for key in ("Occupancy", "ScratchSize"):
            fields[key] = int(re.search(r"; " + key + r": (\d+)", summary).group(1))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="no hipcc")
def test_the_background_ray_rows_kernel_uses_no_scratch_no_lds_and_at_most_128_vgprs(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "background_rays.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "background_rays.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    kernels = _metadata(open(asm).read())
    # NC 1 / 2 / 4 x with or without a grid x with or without t_stop
    assert len(kernels) == 12 and all("background_ray_rows_kernel" in k for k in kernels), sorted(kernels)
    for name, m in sorted(kernels.items()):
        registers = m["vgpr_count"] + m.get("agpr_count", 0)
        derived = min(8, 512 // max(8, (registers + 7) // 8 * 8))
        print(f"{name}: {m['vgpr_count']} VGPRs + {m.get('agpr_count', 0)} AGPRs, scratch {m['private_segment_fixed_size']}, "
              f"LDS {m['group_segment_fixed_size']}, occupancy {m['Occupancy']} (derived {derived})")
        assert m["private_segment_fixed_size"] == 0 and m["ScratchSize"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert registers <= 128, (name, m)
        assert m["Occupancy"] >= 4 and derived >= 4, (name, m)
