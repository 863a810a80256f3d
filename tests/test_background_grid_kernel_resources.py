"""Build-quality gate for the background's rows kernel (csrc/background_rows.hip: background_rows_kernel), CPU only, in the manner
of tests/test_sample_cull_kernel_resources.py and tests/test_termination_kernel_resources.py: hipcc cross-compiles the file to
gfx950 assembly with the flags the build gives it, and the code objects' own metadata is read.

The kernel is launched with __launch_bounds__(256): four waves, one per SIMD of a CU.  It is a latency-bound walk over HBM (the
point, depth and grid-word loads), so it must leave room for at least FOUR workgroups per CU -- at most 128 VGPRs -- and use no
scratch: every ballot of a run is indexed by compile-time constants and lives in registers.
Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): background_rows_kernel<1 | 2 | 4, grid | grid and t_stop>: 39 / 42, 88 / 92 and
27 / 31 VGPRs, occupancy 7, 5 and 7 (the ballots of a run sit in scalar registers)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _kernels(text):
    """{symbol: (VGPRs, scratch bytes, occupancy, LDS bytes)} of every kernel of an assembly listing."""
    out = {}
    for name in re.findall(r"^(_Z\w+):", text, re.M):
        tail = text[text.index(name + ":"):]
        if "s_endpgm" not in tail:
            continue
        body = tail[:tail.index("s_endpgm")]
        get = lambda k: int(re.search(r"; " + k + r": (\d+)", tail).group(1))
        assert "scratch_" not in body and "s_swappc" not in body, name
        out[name] = (get("TotalNumVgprs"), get("ScratchSize"), get("Occupancy"), get("LDSByteSize"))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="no hipcc")
def test_the_background_rows_kernel_uses_no_scratch_and_at_most_128_vgprs(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "background_rows.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "background_rows.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    kernels = _kernels(open(asm).read())
    assert len(kernels) == 6 and all("background_rows_kernel" in k for k in kernels), sorted(kernels)   # NC 1 / 2 / 4 x with or without t_stop
    for name, (vgprs, scratch, occupancy, lds) in sorted(kernels.items()):
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
