"""Build-quality gate for the kernel of early ray termination (csrc/termination.hip: ray_stop_kernel; the rows kernel of
stnerf_visibility_rows is gated by tests/test_sample_rows_kernel_resources.py), CPU only, in the manner of
tests/test_sample_cull_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and
the code objects' own metadata is read.

The kernel is launched with __launch_bounds__(256): four waves, one per SIMD of a CU.  It is a latency-bound walk over HBM (the
merge's dependent loads), so it must leave room for at least FOUR workgroups per CU -- occupancy >= 4 waves per SIMD, i.e. at most
128 VGPRs -- and use no scratch: every per-layer array of the merge (cursors, head depths) is indexed by compile-time constants and
lives in registers.
Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): ray_stop_kernel<4 | 8 | 16>: 34 / 58 / 106 VGPRs, occupancy 8 / 8 / 4."""
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
def test_the_termination_kernels_use_no_scratch_and_fit_four_workgroups_per_cu(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "termination.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "termination.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    kernels = _kernels(open(asm).read())
    assert len(kernels) == 3 and all("ray_stop_kernel" in k for k in kernels), sorted(kernels)       # LCAP 4 / 8 / 16
    for name, (vgprs, scratch, occupancy, lds) in sorted(kernels.items()):
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
