"""Build-quality gate for the listed copy (csrc/layer_cache.hip: copy_layer_raw_listed_kernel), CPU only, in the manner of
tests/test_termination_kernel_resources.py: hipcc cross-compiles the file to gfx950 assembly with the flags the build gives it,
and the code objects' own metadata is read.

The kernel is a copy: one wave per slot, four slots in flight per wave, launched with __launch_bounds__(256).  It is HBM-bound and
hides latency with resident waves, so both flavours (capture, restore) must use no scratch -- the four slots' addresses and values
are indexed by compile-time constants and live in registers --, no LDS, and at most 128 VGPRs (four workgroups per CU at least)."""
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
def test_the_listed_copy_kernels_use_no_scratch_and_at_most_128_vgprs(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "st-nerf_amd", "csrc")
    asm = str(tmp_path / "layer_cache.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "layer_cache.hip")]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL, timeout=900).returncode == 0
    text = open(asm).read()
    kernels = _kernels(text)
    assert len(kernels) == 2 and all("copy_layer_raw_listed_kernel" in k for k in kernels), sorted(kernels)   # capture, restore
    for name, (vgprs, scratch, occupancy, lds) in sorted(kernels.items()):
        print(f"{name}: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}, LDS {lds}")
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
    # a slot's samples move as 16-byte vectors
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
