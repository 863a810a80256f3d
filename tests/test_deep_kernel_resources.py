"""Build-quality gate for the kernels of deep frames (csrc/deep.hip), CPU only, in the manner of
tests/test_occluder_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it, and the
code objects' own metadata is read -- register counts, scratch and LDS, nothing else.

deep_ray_kernel<false> (count) and <true> (fill) walk a ray alike: a layer's t and wM in four blocks in flight before the first
use, ballots for the segment starts; deep_composite_kernel keeps eight sorted rows, their prefix products and eight Af partial sums in
registers.  All must use no scratch and at most 128 VGPRs -- room for four workgroups per CU, the bar of the other helper kernels --
and no LDS beyond the few words the offset scan's workgroups exchange.  Measured with hipcc --offload-arch=gfx950 (ROCm 7.2): count 19
VGPRs, fill 83, composite 103, the three scan kernels 6 / 26 / 26 with 16 / 68 / 16 bytes of LDS."""
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
def test_the_deep_kernels_use_no_scratch_and_at_most_128_vgprs(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "deep.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "deep.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    kernels = _kernels(open(asm).read())
    ray = sorted(k for k in kernels if "deep_ray_kernel" in k)
    composite = [k for k in kernels if "deep_composite_kernel" in k]
    scan = [k for k in kernels if "deep_block_sum_kernel" in k or "select_scan_kernel" in k or "deep_offsets_kernel" in k]
    assert len(ray) == 2 and len(composite) == 1 and len(scan) == 3 and len(kernels) == 6, sorted(kernels)
    for name, (vgprs, scratch, occupancy, lds) in sorted(kernels.items()):
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
        assert lds == 0 if name in ray + composite else lds <= 128, (name, lds)      # only the scan's workgroups exchange words
    from stnerf_amd import build
    assert ("deep.hip", ["-ffp-contract=off"]) in [(s, f) for s, f in build.SOURCES]
