"""Build-quality gate for the two kernels of occluder compositing (csrc/occluder.hip: scene_occluder_kernel,
occluder_stop_kernel), CPU only, in the manner of tests/test_termination_kernel_resources.py: hipcc cross-compiles the file to
gfx950 assembly with the flags the build gives it, and the code objects' own metadata is read.

scene_occluder_kernel is layer_scene_kernel with two sets of sums: HBM-bound, launched with __launch_bounds__(256) over a
persistent grid, every load of a layer (three blocks of t, wM and the raw float4) in flight before the first use, ten accumulators
and the mix in registers.  Both kernels must use no scratch and no LDS and at most 128 VGPRs -- room for four workgroups per CU,
the bar of the other helper kernels.  Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): scene_occluder_kernel 72 VGPRs,
occupancy 7; occluder_stop_kernel 4 VGPRs, occupancy 8."""
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
def test_the_occluder_kernels_use_no_scratch_and_at_most_128_vgprs(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "occluder.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "occluder.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    text = open(asm).read()
    kernels = _kernels(text)
    assert sorted(k for k in kernels if "scene_occluder_kernel" in k or "occluder_stop_kernel" in k) == sorted(kernels) and len(kernels) == 2
    for name, (vgprs, scratch, occupancy, lds) in sorted(kernels.items()):
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
    # the definitions' products and sums stay separate fp32 operations: the file is built without contraction
    assert not re.search(r"\bv_(pk_)?(fma|mac|fmac)\w*_f32", text)
    from stnerf_amd import build
    assert ("occluder.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
